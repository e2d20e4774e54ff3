// Pass planner of qsv_apply_layer / qsv_ensemble_apply_layer (qsv_layer.hip): plain C++17, no HIP types, so that the host
// tests can compile it alone (tests/test_layer_plan_host.py) and the kernels can read the same records.
//
// A PRODUCT LAYER is a 2x2 matrix on each of k distinct index bits of an n-bit register (or of every n-bit member of an
// ensemble).  Its factors commute, so the layer is a set; the STAGES are always applied in ascending bit order, whatever
// order the caller lists them in, and the rounded result is a function of the set alone.
//
// A PASS is a run of consecutive stages whose bits all lie in one TILE of 2^12 amplitudes -- index bits 0..5 (the lanes of
// a wave) and six more -- which k_layer_tile holds in LDS from its load to its store.  Stages are taken greedily, in
// ascending bit order, while at most six distinct bits >= 6 are among them; the six are completed with the lowest unused
// bits in [6, n).  So passes = max(1, ceil(h / 6)), h = the number of stage bits >= 6 (layer_passes).  Registers and
// members of at most 12 bits are one tile of all their bits.  Inside a pass the stages are cut into RUNS of at most four:
// a thread holds the 16 amplitudes of a run's four tile bits in registers, one LDS round trip per run; a short run is
// completed with the highest tile bits it does not use.  Everything is on member-local bits: the plan does not know how
// many members there are, and a tile never leaves a member of 12 bits or more.
//
// The matrices travel as one table [members][k][8 doubles] in stage order (members = 1 where every member takes the same
// matrices): row-major (m00, m01, m10, m11), interleaved complex.  A pass's stages are contiguous in a member's row.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define QSV_LAYER_HD __host__ __device__ inline
#else
#define QSV_LAYER_HD inline
#endif

namespace qsv_layer_plan {

constexpr int LANE_BITS = 6;
constexpr int TILE_BITS = 12;
constexpr int HIGH_BITS = TILE_BITS - LANE_BITS;
constexpr int RUN_BITS = 4;            // tile bits a thread holds in registers (16 amplitudes)
constexpr int MAX_QUBITS = 64;
constexpr int MATRIX_DOUBLES = 8;      // one 2x2 complex matrix

// One pass, passed to the kernels by value as it is: plain data, dword arrays (indexed with scalar loads).
struct Pass {
    int32_t tile_bits;                 // min(n, 12)
    int32_t n_stages;
    int32_t first;                     // the pass's first stage, counted over the whole layer (its place in a table row)
    uint32_t pos[TILE_BITS];           // the tile's index bits, ascending: tile index bit j <-> pos[j]
    // stages in the order they are applied (ascending bits)
    int32_t bit[TILE_BITS];            // the stage's index bit
    int32_t tile_index[TILE_BITS];     // j with pos[j] = bit
    int32_t run[TILE_BITS];            // the run the stage belongs to
    int32_t reg[TILE_BITS];            // its register bit: run_q[run][reg] = tile_index
    int32_t n_runs;
    int32_t run_first[TILE_BITS], run_count[TILE_BITS];
    int32_t run_q[TILE_BITS][RUN_BITS];   // register bits (tile indices) of the run, ascending; min(4, tile_bits) of them
};

struct Layer {
    std::vector<int> order;            // order[s] = the place in the caller's list of stage s
    std::vector<Pass> passes;
};

// ---- the table ---------------------------------------------------------------------------------------------------------
QSV_LAYER_HD uint64_t table_doubles(uint64_t members, int k) { return members * static_cast<uint64_t>(k) * MATRIX_DOUBLES; }
// first double of the matrix of stage `stage` (counted over the whole layer) of member `member`
QSV_LAYER_HD uint64_t table_offset(uint64_t member, int k, int stage) {
    return (member * static_cast<uint64_t>(k) + static_cast<uint64_t>(stage)) * MATRIX_DOUBLES;
}

// ---- pairs of the forms below one tile -----------------------------------------------------------------------------------
// Pair w of a stage on index bit `bit`: the amplitudes insert_zero(w, bit) and that | 1 << bit.  For bit < n and w < 2^(n-1)
// counted inside a member both lie in the member.
QSV_LAYER_HD uint64_t pair_low(uint64_t w, int bit) { return ((w >> bit) << (bit + 1)) | (w & ((1ull << bit) - 1ull)); }
QSV_LAYER_HD uint64_t pair_high(uint64_t w, int bit) { return pair_low(w, bit) | (1ull << bit); }

// passes of a layer on the bits `bits` of an n-bit register or member
inline uint64_t layer_passes(int n, const std::vector<int> &bits) {
    if (bits.empty()) return 0;
    if (n <= TILE_BITS) return 1;
    uint64_t h = 0;
    for (int b : bits) h += b >= LANE_BITS ? 1 : 0;
    return std::max<uint64_t>(1, (h + HIGH_BITS - 1) / HIGH_BITS);
}

// ---- the plan ------------------------------------------------------------------------------------------------------------
// bits[i] = index bit of the caller's i-th factor (distinct, < n <= 64).
inline Layer layer_plan(int n, const std::vector<int> &bits) {
    const int k = static_cast<int>(bits.size());
    Layer out;
    out.order.resize(k);
    for (int i = 0; i < k; ++i) out.order[i] = i;
    std::sort(out.order.begin(), out.order.end(), [&](int x, int y) { return bits[x] < bits[y]; });
    int next = 0;
    while (next < k) {
        // greedy: consecutive stages while at most six distinct bits >= 6 are among them (a tile of all bits when n <= 12)
        uint64_t high = 0;
        int count = 0;
        while (next + count < k) {
            const int b = bits[out.order[next + count]];
            const uint64_t with = b >= LANE_BITS ? high | (1ull << b) : high;
            if (n > TILE_BITS && __builtin_popcountll(with) > HIGH_BITS) break;
            high = with;
            ++count;
        }
        Pass p = {};
        p.tile_bits = std::min(n, TILE_BITS);
        p.n_stages = count;
        p.first = next;
        if (n <= TILE_BITS) {
            for (int j = 0; j < n; ++j) p.pos[j] = static_cast<uint32_t>(j);
        } else {
            for (int b = LANE_BITS; b < n && __builtin_popcountll(high) < HIGH_BITS; ++b) high |= 1ull << b;
            int j = 0;
            for (int b = 0; b < LANE_BITS; ++b) p.pos[j++] = static_cast<uint32_t>(b);
            for (int b = LANE_BITS; b < n; ++b)
                if ((high >> b) & 1) p.pos[j++] = static_cast<uint32_t>(b);
        }
        auto tile_index_of = [&](int b) {
            for (int j = 0; j < p.tile_bits; ++j)
                if (static_cast<int>(p.pos[j]) == b) return j;
            return -1;
        };
        // runs of at most four stages; a short run is completed with the highest tile indices it does not use
        const int width = std::min(RUN_BITS, p.tile_bits);
        for (int first = 0; first < count; first += RUN_BITS) {
            const int u = p.n_runs++, len = std::min(RUN_BITS, count - first);
            p.run_first[u] = first;
            p.run_count[u] = len;
            std::vector<int> q;
            for (int i = 0; i < len; ++i) q.push_back(tile_index_of(bits[out.order[next + first + i]]));
            for (int j = p.tile_bits - 1; static_cast<int>(q.size()) < width; --j)
                if (std::find(q.begin(), q.end(), j) == q.end()) q.push_back(j);
            std::sort(q.begin(), q.end());
            for (int i = 0; i < width; ++i) p.run_q[u][i] = q[i];
            for (int i = 0; i < len; ++i) {
                const int s = first + i;
                p.bit[s] = bits[out.order[next + s]];
                p.tile_index[s] = tile_index_of(p.bit[s]);
                p.run[s] = u;
                for (int r = 0; r < width; ++r)
                    if (q[r] == p.tile_index[s]) p.reg[s] = r;
            }
        }
        out.passes.push_back(p);
        next += count;
    }
    return out;
}

}  // namespace qsv_layer_plan
