// Pass planner of qsv_apply_qft (qsv_qft.hip) and the one statement of its twiddle angles: plain C++17, no HIP types, so
// that the host tests can compile it alone (tests/test_qft_plan_host.py) and the kernels can call the same functions.
//
// The quantum Fourier transform on the ordered qubits q_0 .. q_{m-1} (q_0 most significant, index bit b_r = bit of q_r) is
// m STAGES followed by the reversal of the m qubits.  Stage r is a Hadamard on b_r followed by phases controlled by the
// later qubits: on the pair (a, b) with bit b_r = 0 / 1
//     a' = (a + b) / sqrt 2,     b' = (a - b) t / sqrt 2,     t = exp(2 pi i T_r / 2^L),   L = m - r,
//     T_r(index) = sum_{s > r} bit_{b_s}(index) << (m - 1 - s).
// With X(index) = sum_s bit_{b_s}(index) << (m - 1 - s), the integer the m qubits spell, T_r is X mod 2^(L-1): the ranks
// up to r sit at bits >= L - 1.  So one pass needs X once per amplitude and a mask per stage.
//
// A PASS is a run of consecutive ranks whose bits all lie in one TILE of 2^12 amplitudes -- index bits 0..5 (the lanes of a
// wave) and six more -- which k_qft_tile holds in LDS from its load to its store.  Ranks are taken greedily, in the order
// they are applied, while at most six distinct bits >= 6 are among them; the six are completed with the lowest unused bits
// >= 6.  Inside a pass the stages are cut into RUNS of at most four: a thread holds the 16 amplitudes of a run's four tile
// bits in registers, one LDS round trip per run.  Registers below 2^12 amplitudes are one tile (k_qft_small).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define QSV_QFT_HD __host__ __device__ inline
#else
#define QSV_QFT_HD inline
#endif

namespace qsv_qft_plan {

constexpr int LANE_BITS = 6;
constexpr int TILE_BITS = 12;
constexpr int HIGH_BITS = TILE_BITS - LANE_BITS;
constexpr int RUN_BITS = 4;       // tile bits a thread holds in registers (16 amplitudes)
constexpr int MAX_QUBITS = 64;
enum { INVERSE = 1, NO_SWAPS = 2, CONJUGATE = 4, ALL_FLAGS = 7 };   // QSV_QFT_* of include/qsv.h

// One pass, passed to the kernels by value as it is: plain data, dword arrays (indexed with scalar loads).
struct Pass {
    int32_t tile_bits;                 // min(n, 12)
    int32_t n_stages;
    int32_t twiddle_first;             // inverse: b *= t' first, then the plain butterfly
    int32_t conj_twiddle;              // t' = conj(t): inverse xor conjugate
    double scale;                      // 2^(-n_stages / 2), applied once at the store
    uint32_t pos[TILE_BITS];           // the tile's index bits, ascending (BigArgs::pos order): tile index bit j <-> pos[j]
    // stages in the order they are applied (ranks ascending; descending when twiddle_first)
    int32_t rank[TILE_BITS];
    int32_t tile_index[TILE_BITS];     // j with pos[j] = b_r
    int32_t L[TILE_BITS];              // m - r
    int32_t run[TILE_BITS];            // the run the stage belongs to
    int32_t reg[TILE_BITS];            // its register bit: run_q[run][reg] = tile_index
    int32_t reg_shift[TILE_BITS][RUN_BITS - 1];   // shifts of the run's other register bits, ascending (-1: not a rank)
    // X, split: the ranks whose bit lies in the tile, by tile index, and the others
    int32_t in_shift[TILE_BITS];       // m - 1 - s of the rank s with b_s = pos[j], or -1
    int32_t n_out;
    int32_t out_bit[MAX_QUBITS], out_shift[MAX_QUBITS];
    int32_t n_runs;
    int32_t run_first[TILE_BITS], run_count[TILE_BITS];
    int32_t run_q[TILE_BITS][RUN_BITS];   // register bits (tile indices) of the run, ascending; min(4, tile_bits) of them
};

// ---- the twiddle's angle -------------------------------------------------------------------------------------------------
// t = exp(2 pi i qft_turns / 2^L).  The kernels call the two halves of X and the mask; the host model calls qft_turns.
QSV_QFT_HD uint64_t qft_turns_mask(int L) { return L >= 2 ? (~0ull >> (65 - L)) : 0ull; }   // 2^(L-1) - 1
// X's part from the ranks outside the tile: the same for every amplitude of a tile
QSV_QFT_HD uint64_t qft_turns_out(uint64_t index, const Pass &p) {
    uint64_t x = 0;
    for (int i = 0; i < p.n_out; ++i) x |= ((index >> p.out_bit[i]) & 1ull) << p.out_shift[i];
    return x;
}
// X's part from the ranks inside the tile, from the tile index
QSV_QFT_HD uint64_t qft_turns_in(uint32_t tile_index, const Pass &p) {
    uint64_t x = 0;
    for (int j = 0; j < p.tile_bits; ++j)
        if (p.in_shift[j] >= 0) x |= static_cast<uint64_t>((tile_index >> j) & 1u) << p.in_shift[j];
    return x;
}
QSV_QFT_HD uint32_t qft_tile_index(uint64_t index, const Pass &p) {
    uint32_t t = 0;
    for (int j = 0; j < p.tile_bits; ++j) t |= static_cast<uint32_t>((index >> p.pos[j]) & 1ull) << j;
    return t;
}
// T_r mod 2^L of amplitude `index` for the pass's stage number `stage`: exact for m up to 64
QSV_QFT_HD uint64_t qft_turns(uint64_t index, const Pass &p, int stage) {
    return (qft_turns_out(index, p) | qft_turns_in(qft_tile_index(index, p), p)) & qft_turns_mask(p.L[stage]);
}

// ---- the plan ------------------------------------------------------------------------------------------------------------
// bits[r] = index bit of the transform's qubit r (distinct, < n <= 64).  The reversal is not part of the plan.
inline std::vector<Pass> qft_plan(int n, const std::vector<int> &bits, int flags) {
    const int m = static_cast<int>(bits.size());
    const bool inverse = (flags & INVERSE) != 0, conj = (flags & CONJUGATE) != 0;
    std::vector<int> order(m);                 // ranks in the order they are applied
    for (int i = 0; i < m; ++i) order[i] = inverse ? m - 1 - i : i;
    std::vector<Pass> passes;
    int next = 0;
    while (next < m) {
        // greedy: consecutive ranks while at most six distinct bits >= 6 are among them
        uint64_t high = 0;
        int count = 0;
        while (next + count < m) {
            const int b = bits[order[next + count]];
            const uint64_t with = b >= LANE_BITS ? high | (1ull << b) : high;
            if (__builtin_popcountll(with) > HIGH_BITS) break;
            high = with;
            ++count;
        }
        Pass p = {};
        p.tile_bits = std::min(n, TILE_BITS);
        p.n_stages = count;
        p.twiddle_first = inverse ? 1 : 0;
        p.conj_twiddle = inverse != conj ? 1 : 0;
        p.scale = 1.0;
        for (int i = 0; i < count / 2; ++i) p.scale *= 0.5;
        if (count % 2) p.scale *= 0.70710678118654752440;
        // the tile: every bit of a small register; else bits 0..5, the pass's high bits and the lowest unused bits >= 6
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
        for (int j = 0; j < TILE_BITS; ++j) p.in_shift[j] = -1;
        for (int s = 0; s < m; ++s) {
            const int j = tile_index_of(bits[s]);
            if (j >= 0) {
                p.in_shift[j] = m - 1 - s;
            } else {
                p.out_bit[p.n_out] = bits[s];
                p.out_shift[p.n_out] = m - 1 - s;
                ++p.n_out;
            }
        }
        // runs of at most four stages; a short run is completed with the highest tile indices it does not use (row bits
        // where it can: the lanes of a wave then read consecutive amplitudes)
        const int width = std::min(RUN_BITS, p.tile_bits);
        for (int first = 0; first < count; first += RUN_BITS) {
            const int u = p.n_runs++, len = std::min(RUN_BITS, count - first);
            p.run_first[u] = first;
            p.run_count[u] = len;
            std::vector<int> q;
            for (int i = 0; i < len; ++i) q.push_back(tile_index_of(bits[order[next + first + i]]));
            for (int j = p.tile_bits - 1; static_cast<int>(q.size()) < width; --j)
                if (std::find(q.begin(), q.end(), j) == q.end()) q.push_back(j);
            std::sort(q.begin(), q.end());
            for (int k = 0; k < width; ++k) p.run_q[u][k] = q[k];
            for (int i = 0; i < len; ++i) {
                const int s = first + i, r = order[next + s];
                p.rank[s] = r;
                p.tile_index[s] = tile_index_of(bits[r]);
                p.L[s] = m - r;
                p.run[s] = u;
                int others = 0;
                for (int k = 0; k < RUN_BITS - 1; ++k) p.reg_shift[s][k] = -1;
                for (int k = 0; k < width; ++k) {
                    if (q[k] == p.tile_index[s])
                        p.reg[s] = k;
                    else
                        p.reg_shift[s][others++] = p.in_shift[q[k]];
                }
            }
        }
        passes.push_back(p);
        next += count;
    }
    return passes;
}

// The reversal as qsvk_permute takes it: destination bit d takes source bit src[d]; true if it moves anything.
inline bool qft_reversal(int n, const std::vector<int> &bits, int *src_bit_of_dst_bit) {
    const int m = static_cast<int>(bits.size());
    for (int b = 0; b < n; ++b) src_bit_of_dst_bit[b] = b;
    for (int r = 0; r < m; ++r) src_bit_of_dst_bit[bits[r]] = bits[m - 1 - r];
    return m >= 2;
}

}  // namespace qsv_qft_plan
