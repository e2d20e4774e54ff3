// Reversible register arithmetic (qsv_apply_arith): everything that is not device code.  Plain C++17,
// included by qsv_arith.hip and by the host tests (tests/layout/arith_layout_driver.cpp): the operand segments, the choice
// of form, the launch shape, the reciprocal and the reduction, modular inverses, table inversion, the validation of a
// handle's parameters and the kernel-argument struct.  arith_source() below is the kernel's whole index computation; the
// kernel calls it per work item and the host tests call it per basis index, so the two cannot drift apart.
//
// The maps.  A map acts on the value y that m target bits spell (value bit j at some index bit), may read the value x of
// mx source bits, and acts only where every control bit is 1.  M is the modulus (M = 2^m allowed); y >= M stays.  On a state
// vector the map is a permutation of amplitudes and the kernel gathers: dst[i] = src[i with y replaced by g(y, x)], g the
// INVERSE of the map asked for.  Four bodies cover the six kinds and their inverses:
//     SHIFT   g = y + (c + a x mod M) mod M        ADD, ADD_REG
//     MULT    g = f y mod M, f = a or table[x]     MUL, MUL_POW
//     XOR     g = y xor table[x]                   XOR_LOOKUP
//     TABLE   g = table[y]                         PERMUTE
//
// The reduction.  No 64-bit division on the device.  With R = floor(2^64 / M), 2 <= M <= 2^32, and any p < 2^64:
//     q = floor(p R / 2^64)           (the high word of the 128-bit product)
// satisfies Q - 1 <= q <= Q for Q = floor(p / M).  Proof: R = 2^64 / M - e with 0 <= e < 1, so p R / 2^64 = p / M - p e / 2^64,
// and 0 <= p e / 2^64 < 1.  Hence p / M - 1 < p R / 2^64 <= p / M; the floor of the right side is Q and the floor of anything
// above Q - 1 is at least Q - 1.  So p - q M lies in [0, 2 M) -- below 2^33, no overflow -- and ONE conditional subtraction
// finishes.  Both operands of every product are below M <= 2^32 (f, y, a) or below 2^32 (x), so p < 2^64 always.  SHIFT adds
// c (< M) to a reduced a x and y (< M) to the sum: one more conditional subtraction each.  M = 2^m needs a mask only and is
// a separate instantiation (POW2).
//
// The forms.  Source and control bits are read, not moved: source and destination index differ in target bits alone.  But a
// source or control bit below bit 3 makes the lanes of one 128-byte destination line evaluate different maps, so the line is
// gathered from several source lines just as with a low target bit.  With the lowest target, source and control bit d0 >= 3
// every destination line comes from one whole source line (the LINE form); with d0 < 3 reads come in runs of 2^d0 amplitudes
// (the ELEMENT form).  Both are the same kernel -- a wave stores 64 consecutive amplitudes and loads wherever the map
// points -- so the ELEMENT form is correct for every placement by construction; the names say what the memory system sees
// and go into last_kernel.  Measured on 28 qubits (profiles/r20_arith.json; a copy takes 1.32 ms, the
// bit-reversal permutation 1.66 ms): LINE runs at 0.99 to 1.16 x the time of a copy, below the permutation; ELEMENT with
// a low target at 1.04 to 1.12 x for additions and multiplications (neighbouring values mostly land in neighbouring lines,
// which the caches absorb) and 1.86 x for a random table on bits 0 .. 8; with a control on bit 0 at 1.47 x; and at 2.81 x in
// the worst case met, a source on bits 0 .. 9 that sends every lane to a line of its own.  A route that moves the low bits
// away with qsvk_permute, runs the LINE form and moves them back costs two permutations and a LINE pass, 3.5 x a copy: it
// loses in every case measured.  It is NOT built.
// Amplitudes that differ only in spectator bits can share one evaluation of the map: a lane may take 2^items_log2 of them,
// the lowest spectator bits at or above bit 6, so every item of a wave is still 64 consecutive amplitudes.  Measured, ONE
// amplitude per lane is fastest (LINE multiply 1.03 x copy against 1.07 with two and 1.12 with four; target on bit 0: 1.10 /
// 1.11 / 1.21), as for the copy kernel itself (qsv_device.h, ro_move_items): the index arithmetic is not what a pass waits
// for.  So the default is one, and QSV_ARITH_ITEMS = 1 / 2 raises the cap to two / four for measurements.  Registers below
// the stream threshold (14 qubits, as in qsv_readout_layout.h) always take one amplitude per lane (SMALL).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define QSV_ARITH_HD __host__ __device__ inline
#else
#define QSV_ARITH_HD inline
#endif

namespace qsv_arith_layout {

enum Kind { KIND_ADD = 0, KIND_MUL = 1, KIND_ADD_REG = 2, KIND_MUL_POW = 3, KIND_XOR_LOOKUP = 4, KIND_PERMUTE = 5, KIND_COUNT = 6 };
enum Body { BODY_SHIFT = 0, BODY_MULT = 1, BODY_XOR = 2, BODY_TABLE = 3 };
enum Form { FORM_SMALL = 0, FORM_LINE = 1, FORM_ELEMENT = 2 };

constexpr int ARITH_BLOCK = 256;            // = QSV_BLOCK
constexpr int ARITH_MAX_BITS = 32;          // widest target and source operand
constexpr int ARITH_MAX_TABLE_BITS = 24;    // widest table index (64 MiB of 32-bit words)
constexpr int ARITH_STREAM_QUBITS = 14;     // = RO_MIN_QUBITS
constexpr int ARITH_LANE_BITS = 6;          // = QSV_LANE_BITS
constexpr int ARITH_MAX_ITEMS_LOG2 = 2;
constexpr int ARITH_DEFAULT_ITEMS_LOG2 = 0;  // one amplitude per lane: the fastest measured (see above)
constexpr uint32_t ARITH_GRID_CAP = 1u << 20;   // x 256 threads = 2^28 work-items per dispatch, far below the 2^32 of an AQL packet
constexpr int ARITH_INVERSE = 1;            // = QSV_ARITH_INVERSE

inline const char *body_name(int body) {
    static const char *const names[] = {"shift", "mult", "xor", "table"};
    return names[body & 3];
}
inline const char *form_name(int form) {
    static const char *const names[] = {"small", "line", "element"};
    return names[form % 3];
}

// ---- the reduction ---------------------------------------------------------------------------------------------------
QSV_ARITH_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

// floor(2^64 / M) for 2 <= M <= 2^32
inline uint64_t reciprocal(uint64_t M) {
    const uint64_t q = ~0ull / M, r = ~0ull % M;      // 2^64 - 1 = q M + r
    return r + 1 == M ? q + 1 : q;
}

// p mod M for any p < 2^64, R = reciprocal(M) (the proof is at the top of this file)
QSV_ARITH_HD uint64_t reduce(uint64_t p, uint64_t M, uint64_t R) {
    const uint64_t r = p - mulhi64(p, R) * M;
    return r >= M ? r - M : r;
}

inline uint64_t gcd(uint64_t a, uint64_t b) {
    while (b) {
        const uint64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// a^-1 mod M for gcd(a, M) = 1, 0 < a < M <= 2^32 (M = 2 with a = 1 included); 0 when there is none
inline uint64_t mod_inverse(uint64_t a, uint64_t M) {
    int64_t r0 = static_cast<int64_t>(M), r1 = static_cast<int64_t>(a % M), t0 = 0, t1 = 1;
    while (r1) {
        const int64_t q = r0 / r1, r2 = r0 - q * r1, t2 = t0 - q * t1;
        r0 = r1, r1 = r2, t0 = t1, t1 = t2;
    }
    if (r0 != 1) return 0;
    return static_cast<uint64_t>(t0 < 0 ? t0 + static_cast<int64_t>(M) : t0);
}

// inv[table[y]] = y; false if table is not a bijection of 0 .. size-1
inline bool invert_table(const std::vector<uint32_t> &table, std::vector<uint32_t> *inv) {
    const size_t size = table.size();
    std::vector<uint8_t> seen(size, 0);
    inv->assign(size, 0);
    for (size_t y = 0; y < size; ++y) {
        if (table[y] >= size || seen[table[y]]) return false;
        seen[table[y]] = 1;
        (*inv)[table[y]] = static_cast<uint32_t>(y);
    }
    return true;
}

// ---- a handle's parameters -------------------------------------------------------------------------------------------
// One parameter set = what the gather needs for one direction.
struct Set {
    int body = BODY_SHIFT;
    uint64_t a = 0, c = 0;            // SHIFT: s = c + a x; MULT without table: f = a
    std::vector<uint32_t> table;      // MULT: f = table[x]; XOR: table[x]; TABLE: table[y]
    bool identity = false;            // the map moves nothing: no launch
};

struct Params {
    int kind = 0, m = 0, mx = 0;
    uint64_t M = 0;                   // the modulus, 2^m spelled out
    bool pow2 = false;                // M == 2^m
    uint64_t recip = 0;
    Set gather_fwd, gather_inv;       // what the kernel gathers with to apply the map / its inverse
};

// Checks everything qsv_arith_create refuses and fills *out; nullptr = accepted, otherwise the message.
inline const char *make_params(int kind, int m, int mx, uint64_t a, uint64_t c, uint64_t modulus, const uint64_t *table,
                               uint64_t table_len, Params *out) {
    if (kind < 0 || kind >= KIND_COUNT) return "unknown kind of register map";
    const bool has_source = kind == KIND_ADD_REG || kind == KIND_MUL_POW || kind == KIND_XOR_LOOKUP;
    const bool has_table = kind == KIND_XOR_LOOKUP || kind == KIND_PERMUTE;
    const bool modular = kind != KIND_XOR_LOOKUP && kind != KIND_PERMUTE;
    if (m < 1 || m > (kind == KIND_PERMUTE ? ARITH_MAX_TABLE_BITS : ARITH_MAX_BITS)) return "target width m out of range";
    if (has_source) {
        if (mx < 1 || mx > (kind == KIND_ADD_REG ? ARITH_MAX_BITS : ARITH_MAX_TABLE_BITS)) return "source width mx out of range";
    } else if (mx != 0) {
        return "this kind of map reads no source register: mx must be 0";
    }
    const uint64_t full = 1ull << m;
    uint64_t M = full;
    if (modular) {
        if (modulus != 0) M = modulus;
        if (M < 2 || M > full) return "modulus must be in 2 .. 2^m (0 stands for 2^m)";
    } else if (modulus != 0) {
        return "this kind of map has no modulus";
    }
    const bool uses_a = kind == KIND_MUL || kind == KIND_ADD_REG || kind == KIND_MUL_POW;
    const bool uses_c = kind == KIND_ADD || kind == KIND_ADD_REG;
    if (uses_a ? a >= M : a != 0) return uses_a ? "multiplier a must be below the modulus" : "this kind of map has no multiplier a";
    if (uses_c ? c >= M : c != 0) return uses_c ? "constant c must be below the modulus" : "this kind of map has no constant c";
    if (has_table) {
        if (!table) return "this kind of map needs a table";
        if (table_len != 1ull << (kind == KIND_PERMUTE ? m : mx)) return "wrong table length";
        for (uint64_t i = 0; i < table_len; ++i)
            if (table[i] >= full) return "table entry out of range";
    } else if (table || table_len) {
        return "this kind of map takes no table";
    }
    uint64_t a_inv = 0;
    if (kind == KIND_MUL || kind == KIND_MUL_POW) {
        if (gcd(a, M) != 1) return "multiplier a must be coprime to the modulus";
        a_inv = mod_inverse(a, M);
    }
    Params p;
    p.kind = kind, p.m = m, p.mx = mx, p.M = M, p.pow2 = M == full, p.recip = reciprocal(M);
    Set fwd, inv;        // the map and its inverse, as gathers of their own
    switch (kind) {
        case KIND_ADD:
        case KIND_ADD_REG:
            fwd.body = inv.body = BODY_SHIFT;
            fwd.a = a, fwd.c = c;
            inv.a = (M - a) % M, inv.c = (M - c) % M;
            fwd.identity = inv.identity = a == 0 && c == 0;
            break;
        case KIND_MUL:
            fwd.body = inv.body = BODY_MULT;
            fwd.a = a, inv.a = a_inv;
            fwd.identity = inv.identity = a == 1;
            break;
        case KIND_MUL_POW: {
            fwd.body = inv.body = BODY_MULT;
            const uint64_t len = 1ull << mx;
            fwd.table.resize(len), inv.table.resize(len);
            uint64_t f = 1 % M, g = 1 % M;
            for (uint64_t x = 0; x < len; ++x) {
                fwd.table[x] = static_cast<uint32_t>(f), inv.table[x] = static_cast<uint32_t>(g);
                f = f * a % M, g = g * a_inv % M;        // host code: both factors below 2^32
            }
            fwd.identity = inv.identity = a == 1;
            break;
        }
        case KIND_XOR_LOOKUP:
            fwd.body = inv.body = BODY_XOR;
            fwd.table.assign(table, table + table_len);
            inv.table = fwd.table;
            fwd.identity = inv.identity = std::all_of(fwd.table.begin(), fwd.table.end(), [](uint32_t v) { return v == 0; });
            break;
        default: {
            fwd.body = inv.body = BODY_TABLE;
            fwd.table.assign(table, table + table_len);
            if (!invert_table(fwd.table, &inv.table)) return "the table is not a bijection";
            bool same = true;
            for (uint64_t y = 0; y < table_len; ++y) same = same && fwd.table[y] == y;
            fwd.identity = inv.identity = same;
        }
    }
    // applying a map = gathering with its inverse
    p.gather_fwd = std::move(inv);
    p.gather_inv = std::move(fwd);
    *out = std::move(p);
    return nullptr;
}

// ---- operands as segments ----------------------------------------------------------------------------------------------
// Value bits j .. j+len-1 of an operand sit at index bits pos .. pos+len-1.  One 32-bit word each (a dword array in the
// kernarg segment is read with scalar loads): pos | j << 8 | len << 16.
QSV_ARITH_HD uint32_t seg_pos(uint32_t s) { return s & 255u; }
QSV_ARITH_HD uint32_t seg_j(uint32_t s) { return (s >> 8) & 255u; }
QSV_ARITH_HD uint32_t seg_len(uint32_t s) { return s >> 16; }

// bits[r] = index bit of the operand's qubit r, most significant first: value bit j is index bit bits[count - 1 - j].
// Neighbouring value bits at neighbouring index bits merge; a contiguous operand is one segment.
inline std::vector<uint32_t> segments(const int *bits, int count) {
    std::vector<uint32_t> out;
    for (int j = 0; j < count;) {
        const int pos = bits[count - 1 - j];
        int len = 1;
        while (j + len < count && bits[count - 1 - (j + len)] == pos + len) ++len;
        out.push_back(static_cast<uint32_t>(pos) | static_cast<uint32_t>(j) << 8 | static_cast<uint32_t>(len) << 16);
        j += len;
    }
    return out;
}

// ---- kernel arguments ----------------------------------------------------------------------------------------------------
struct ArithArgs {
    uint64_t W;          // work items: amplitudes >> items_log2
    uint64_t cmask;      // control bits: the map acts where (i & cmask) == cmask
    uint64_t tmask;      // the target's index bits
    uint64_t M, recip;   // modulus and floor(2^64 / M)
    uint64_t a, c;
    uint64_t ymask;      // 2^m - 1
    int32_t n_tseg, n_sseg;
    int32_t items_log2;
    int32_t item_bit[ARITH_MAX_ITEMS_LOG2];   // the spectator bits a lane's items differ in, ascending
    int32_t has_table;   // MULT: f = table[x] instead of a
    uint32_t tseg[ARITH_MAX_BITS], sseg[ARITH_MAX_BITS];
};
static_assert(sizeof(ArithArgs) == 8 * 8 + 6 * 4 + 2 * 4 * ARITH_MAX_BITS, "ArithArgs has no padding: 344 bytes of kernarg");

QSV_ARITH_HD uint64_t extract(uint64_t i, const uint32_t *seg, int n_seg) {
    uint64_t v = 0;
    for (int k = 0; k < n_seg; ++k) {
        const uint32_t s = seg[k];
        v |= ((i >> seg_pos(s)) & ((1ull << seg_len(s)) - 1ull)) << seg_j(s);
    }
    return v;
}
QSV_ARITH_HD uint64_t scatter(uint64_t v, const uint32_t *seg, int n_seg) {
    uint64_t i = 0;
    for (int k = 0; k < n_seg; ++k) {
        const uint32_t s = seg[k];
        i |= ((v >> seg_j(s)) & ((1ull << seg_len(s)) - 1ull)) << seg_pos(s);
    }
    return i;
}

QSV_ARITH_HD uint64_t insert_zero_bit(uint64_t w, int p) {
    const uint64_t low = w & ((1ull << p) - 1ull);
    return ((w >> p) << (p + 1)) | low;
}

// work item w -> the index of its first amplitude: zeros at the item bits
QSV_ARITH_HD uint64_t arith_base(uint64_t w, const ArithArgs &g) {
    for (int k = 0; k < g.items_log2; ++k) w = insert_zero_bit(w, g.item_bit[k]);
    return w;
}

// The index dst[i] is read from.  BODY and POW2 are compile-time in the kernel.
template <int BODY, bool POW2>
QSV_ARITH_HD uint64_t arith_source(uint64_t i, const ArithArgs &g, const uint32_t *table) {
    if ((i & g.cmask) != g.cmask) return i;
    const uint64_t y = extract(i, g.tseg, g.n_tseg);
    if (!POW2 && y >= g.M) return i;
    uint64_t x = 0;
    if (BODY != BODY_TABLE) x = extract(i, g.sseg, g.n_sseg);
    uint64_t out;
    if (BODY == BODY_SHIFT) {
        if (POW2) {
            out = (y + g.c + g.a * x) & g.ymask;
        } else {
            uint64_t s = reduce(g.a * x, g.M, g.recip) + g.c;
            if (s >= g.M) s -= g.M;
            out = y + s;
            if (out >= g.M) out -= g.M;
        }
    } else if (BODY == BODY_MULT) {
        const uint64_t f = g.has_table ? table[x] : g.a;
        out = POW2 ? (f * y) & g.ymask : reduce(f * y, g.M, g.recip);
    } else if (BODY == BODY_XOR) {
        out = y ^ table[x];
    } else {
        out = table[y];
    }
    return (i & ~g.tmask) | scatter(out, g.tseg, g.n_tseg);
}

// ---- form and launch shape ---------------------------------------------------------------------------------------------
struct Shape {
    int form = FORM_SMALL;
    int items_log2 = 0;
    int item_bit[ARITH_MAX_ITEMS_LOG2] = {0, 0};
    uint64_t W = 1;
    uint32_t grid = 1;     // workgroups of ARITH_BLOCK threads; the kernel strides over W, so grid x block < 2^32 whatever n is
};

// lowest_bit: the lowest index bit among target, source and controls
inline int choose_form(int n, int lowest_bit) {
    if (n < ARITH_STREAM_QUBITS) return FORM_SMALL;
    return lowest_bit >= 3 ? FORM_LINE : FORM_ELEMENT;
}

// used = every target, source and control bit (never empty); max_items_log2: 0 .. ARITH_MAX_ITEMS_LOG2
inline Shape launch_shape(int n, uint64_t used, int max_items_log2) {
    Shape s;
    int d0 = 0;
    while (d0 < 63 && !((used >> d0) & 1ull)) ++d0;
    s.form = choose_form(n, d0);
    if (s.form != FORM_SMALL)
        for (int b = ARITH_LANE_BITS; b < n && s.items_log2 < std::min(max_items_log2, ARITH_MAX_ITEMS_LOG2); ++b)
            if (!((used >> b) & 1ull)) s.item_bit[s.items_log2++] = b;
    s.W = (1ull << n) >> s.items_log2;
    const uint64_t blocks = (s.W + ARITH_BLOCK - 1) / ARITH_BLOCK;
    s.grid = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(blocks, 1), ARITH_GRID_CAP));
    return s;
}

// Everything of the kernel's arguments that depends on the call: tbits / sbits / cbits are index bits, most significant
// operand qubit first.
inline ArithArgs make_args(const Params &p, const Set &set, const Shape &shape, const int *tbits, const int *sbits, int n_controls,
                           const int *cbits) {
    ArithArgs g = {};
    g.W = shape.W;
    for (int k = 0; k < n_controls; ++k) g.cmask |= 1ull << cbits[k];
    for (int r = 0; r < p.m; ++r) g.tmask |= 1ull << tbits[r];
    g.M = p.M, g.recip = p.recip, g.a = set.a, g.c = set.c;
    g.ymask = (1ull << p.m) - 1ull;
    const std::vector<uint32_t> t = segments(tbits, p.m), s = segments(sbits, p.mx);
    g.n_tseg = static_cast<int32_t>(t.size()), g.n_sseg = static_cast<int32_t>(s.size());
    std::copy(t.begin(), t.end(), g.tseg);
    std::copy(s.begin(), s.end(), g.sseg);
    g.items_log2 = shape.items_log2;
    for (int k = 0; k < ARITH_MAX_ITEMS_LOG2; ++k) g.item_bit[k] = shape.item_bit[k];
    g.has_table = set.body == BODY_MULT && !set.table.empty();
    return g;
}

inline uint64_t used_mask(int m, const int *tbits, int mx, const int *sbits, int n_controls, const int *cbits) {
    uint64_t used = 0;
    for (int r = 0; r < m; ++r) used |= 1ull << tbits[r];
    for (int r = 0; r < mx; ++r) used |= 1ull << sbits[r];
    for (int k = 0; k < n_controls; ++k) used |= 1ull << cbits[k];
    return used;
}

}  // namespace qsv_arith_layout
