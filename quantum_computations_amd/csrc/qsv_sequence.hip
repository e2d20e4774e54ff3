// Fused gate blocks applied as the SEQUENCE of their source gates: on the 32 amplitudes a thread holds (k_seq_big,
// k_seq_lds; qsvk_sequence5) and on LDS-resident tiles of 4096 amplitudes (k_seq_tile; qsvk_sequence_tile).  The dense
// forms of the same blocks are qsv_gatek.hip; the records and the pass cutter are qsv_layout.h.

#include "qsv_internal.h"
#include "qsv_device.h"
#include "qsv_layout.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace qsv_layout;   // the argument and record types of the kernels, and the host-side tables the launchers fill them from

namespace {

// ----------------------------------------------------------------------------------------------------
// Fused 5-qubit blocks as a SEQUENCE of their source gates (round 3).  A dense 32 x 32 complex block costs 4 x 1024 real
// FMAs per amplitude group -- the one shape of the gate path that is bound by arithmetic (the vector pipe is 81 % busy at
// the clock its power draw leaves it: profiles/r03_k5_sq_counters.txt).  But a fused block IS a product of a few 1- and
// 2-qubit gates (5.9 on average on the benchmark circuit): applied one after the other to the 32 amplitudes a thread
// already holds in registers they cost 256 FMAs per 1-qubit gate and 512 per 2-qubit gate, ~2 400 per block instead of
// 4 096, and nothing but the gates' own small matrices comes through the scalar cache.  Loads, the exchange of low target bits
// (address arithmetic for lane bits 3..5, the XOR-swizzled LDS rows for bits 0..2) and stores are k_dense_big's /
// k_dense_lds's; only the arithmetic in the middle differs.  The register index is runtime data of the gate list, the
// register ARRAY must be indexed statically: one unrolled body per register bit (1-qubit gates) and per pair of register
// bits (2-qubit gates, leg 0 canonicalised onto the higher bit by the host), selected by a wave-uniform switch.
// ----------------------------------------------------------------------------------------------------
static int seq_max_work() {
    static const int v = [] {
        const char *e = getenv("QSV_SEQUENCE_WORK");
        return e ? atoi(e) : 0;      // measured (profiles/r03_sequence_blocks.txt): no faster than the dense block
    }();
    return v;
}

template <int J, int D = 32>
__device__ __forceinline__ void seq_apply1(amp_t (&x)[D], const double *__restrict__ m) {
    const cplx m00{m[0], m[1]}, m01{m[2], m[3]}, m10{m[4], m[5]}, m11{m[6], m[7]};
#pragma unroll
    for (int c = 0; c < D; ++c) {
        if (c & (1 << J)) continue;
        const amp_t a0 = x[c], a1 = x[c | (1 << J)];
        x[c] = cfma(m01, a1, cmul(m00, a0));
        x[c | (1 << J)] = cfma(m11, a1, cmul(m10, a0));
    }
}

template <int HI, int LO, int D = 32>
__device__ __forceinline__ void seq_apply2(amp_t (&x)[D], const double *__restrict__ m) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
        if (c & ((1 << HI) | (1 << LO))) continue;
        const amp_t in[4] = {x[c], x[c | (1 << LO)], x[c | (1 << HI)], x[c | (1 << HI) | (1 << LO)]};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            amp_t acc = cmul(cplx{m[8 * r], m[8 * r + 1]}, in[0]);
#pragma unroll
            for (int cc = 1; cc < 4; ++cc) acc = cfma(cplx{m[8 * r + 2 * cc], m[8 * r + 2 * cc + 1]}, in[cc], acc);
            x[c | ((r >> 1) << HI) | ((r & 1) << LO)] = acc;
        }
    }
}

__device__ __forceinline__ void seq_run(amp_t (&x)[32], const SeqGate *__restrict__ gates, int n_gates) {
#pragma unroll 1
    for (int g = 0; g < n_gates; ++g) {
        const double *m = gates[g].m;
        switch (gates[g].code) {     // wave-uniform (scalar loads)
            case 0: seq_apply1<0>(x, m); break;
            case 1: seq_apply1<1>(x, m); break;
            case 2: seq_apply1<2>(x, m); break;
            case 3: seq_apply1<3>(x, m); break;
            case 4: seq_apply1<4>(x, m); break;
            case 5: seq_apply2<1, 0>(x, m); break;
            case 6: seq_apply2<2, 0>(x, m); break;
            case 7: seq_apply2<2, 1>(x, m); break;
            case 8: seq_apply2<3, 0>(x, m); break;
            case 9: seq_apply2<3, 1>(x, m); break;
            case 10: seq_apply2<3, 2>(x, m); break;
            case 11: seq_apply2<4, 0>(x, m); break;
            case 12: seq_apply2<4, 1>(x, m); break;
            case 13: seq_apply2<4, 2>(x, m); break;
            default: seq_apply2<4, 3>(x, m); break;
        }
    }
}

// every target on bit 6 or higher: k_dense_big<5, 0>'s loads and in-place stores around the gate sequence
template <bool NT>
__global__ __launch_bounds__(QSV_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_seq_big(amp_t *__restrict__ a, const BigArgs g, const SeqGate *__restrict__ gates,
                                                      int n_gates, const uint64_t *__restrict__ hoff) {
    constexpr int D = 32;
    const uint64_t tile = (g.regions > 1 && gridDim.x % g.regions == 0)
                              ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                              : blockIdx.x;
    const uint64_t w = g.w0 + tile * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x;
    if (w >= g.W) return;
    const uint64_t base = deposit(w, g);
    amp_t x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = ld<NT>(a + base + hoff[c]);
    seq_run(x, gates, n_gates);
#pragma unroll
    for (int c = 0; c < D; ++c) st<NT>(a + base + hoff[c], x[c]);
}

// targets below bit 6: k_dense_lds<5, KB>'s addressing and LDS exchange around the gate sequence
template <int KB, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_seq_lds(amp_t *__restrict__ a, const LdsArgs g, const SeqGate *__restrict__ gates,
                                                      int n_gates, const uint64_t *__restrict__ hoff) {
    constexpr int D = 32, NB = 1 << KB;
    __shared__ amp_t tiles[KB > 0 ? NB * QSV_BLOCK : 1];
    amp_t *tile = tiles + (KB > 0 ? NB * 64 * (threadIdx.x >> 6) : 0);
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    const uint64_t w = g.w0 + tile_id * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x;
    if (w >= g.W) return;  // W and w0 are multiples of 64: whole waves leave together
    const uint32_t lane = threadIdx.x & 63;
    uint64_t base = deposit(w, g) & ~static_cast<uint64_t>(g.amask);
    for (int j = 0; j < g.na; ++j) base |= static_cast<uint64_t>((lane >> g.abit[j]) & 1u) << g.aE[j];
    amp_t x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = ld<NT>(a + base + hoff[c]);
    uint32_t my_row = 0;
    if constexpr (KB > 0) {
#pragma unroll
        for (int v = 1; v < NB; ++v)
            if ((lane & g.bmask) == g.bdep[v]) my_row = v;
#pragma unroll
        for (int o = 0; o < D / NB; ++o) {
            wave_sync();
#pragma unroll
            for (int s = 0; s < NB; ++s) tile[s * 64 + (lane ^ g.bdep[s])] = x[o * NB + s];
            wave_sync();
#pragma unroll
            for (int t = 0; t < NB; ++t) x[o * NB + t] = tile[my_row * 64 + (lane ^ g.bdep[t])];
        }
    }
    seq_run(x, gates, n_gates);
    if constexpr (KB > 0) {
#pragma unroll
        for (int o = 0; o < D / NB; ++o) {
            wave_sync();
#pragma unroll
            for (int t = 0; t < NB; ++t) tile[my_row * 64 + (lane ^ g.bdep[t])] = x[o * NB + t];
            wave_sync();
#pragma unroll
            for (int s = 0; s < NB; ++s) st<NT>(a + base + hoff[o * NB + s], tile[s * 64 + (lane ^ g.bdep[s])]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < D; ++c) st<NT>(a + base + hoff[c], x[c]);
    }
}

}  // namespace

// ---- a fused block as the SEQUENCE of its source gates on an LDS-resident tile (round 3) -------------------------------
// Dense 5- and 6-qubit blocks are the gate shapes bound by arithmetic (4 x 32 / 3 x 64 real multiply-adds per amplitude at
// a power-limited clock: 1.6 / 1.9 ms against the 1.31 ms of a pass over HBM), yet a fused block is the product of a
// handful of 1- and 2-qubit gates worth 4-8 multiply-adds each.  Here a workgroup brings a 4096-amplitude tile into LDS
// -- the block's K target bits plus the 12 - K lowest other bits: every row of the tile is 64 contiguous amplitudes (bits
// 0-5 are always in the tile when K <= 6), so HBM sees whole 1 KiB runs in both directions, straight into LDS on the way
// in -- and applies the source gates one after the other on that 12-qubit register (a barrier between gates), as the
// single-launch executor does with whole registers (qsv_circuit.hip).  Two workgroups per CU: one computes while the
// other loads or stores.
// The gate list is cut into PASSES over at most four tile bits each (consecutive gates whose legs fit four bits together):
// a thread takes the 16 amplitudes of one group of the pass's four bits into registers, applies the pass's gates there
// (seq_apply*: compile-time register indices behind a wave-uniform switch) and puts them back -- one LDS round trip and one
// barrier per pass instead of one per gate.

constexpr int TILE_SEQ_ROWS_PER_WAVE = TILE_SEQ_ROWS / (TILE_SEQ_THREADS / 64);

struct TileSeqArgs {
    BigArgs g;              // pos[] = ALL tile bits: the tile number is deposited around them
    uint32_t lane_bit[6];   // address bit of lane bit j (the six lowest tile bits: 0..5 unless a 6-qubit block sits above them)
};

__device__ __forceinline__ void seq_run16(amp_t (&x)[16], const SeqGate *__restrict__ gates, int n_gates) {
#pragma unroll 1
    for (int g = 0; g < n_gates; ++g) {
        const double *m = gates[g].m;
        switch (gates[g].code) {     // wave-uniform (scalar loads): 0..3 one-qubit gates, 5 + p two-qubit gates as in SeqGate
            case 0: seq_apply1<0, 16>(x, m); break;
            case 1: seq_apply1<1, 16>(x, m); break;
            case 2: seq_apply1<2, 16>(x, m); break;
            case 3: seq_apply1<3, 16>(x, m); break;
            case 5: seq_apply2<1, 0, 16>(x, m); break;
            case 6: seq_apply2<2, 0, 16>(x, m); break;
            case 7: seq_apply2<2, 1, 16>(x, m); break;
            case 8: seq_apply2<3, 0, 16>(x, m); break;
            case 9: seq_apply2<3, 1, 16>(x, m); break;
            default: seq_apply2<3, 2, 16>(x, m); break;
        }
    }
}

template <bool NT>
__global__ __launch_bounds__(TILE_SEQ_THREADS) void k_seq_tile(amp_t *__restrict__ a, const TileSeqArgs ta,
                                                              const SeqGate *__restrict__ gates,
                                                              const TilePass *__restrict__ passes, int n_passes,
                                                              const uint64_t *__restrict__ off) {   // [rows] row offsets
    const BigArgs &g = ta.g;
    extern __shared__ __attribute__((aligned(16))) char seq_smem[];
    amp_t *tile = reinterpret_cast<amp_t *>(seq_smem);        // [rows][64 lanes] = the tile register, index row * 64 + lane
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave q: rows q RPW .. q RPW + RPW - 1
    constexpr int RPW = TILE_SEQ_ROWS_PER_WAVE;
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    uint64_t base = deposit(g.w0 + tile_id, g);
#pragma unroll
    for (int j = 0; j < 6; ++j) base |= static_cast<uint64_t>((lane >> j) & 1) << ta.lane_bit[j];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < RPW; ++i)
        __builtin_amdgcn_global_load_lds(a + base + off[q * RPW + i], tile + (q * RPW + i) * 64, 16, 0, NT ? 2 : 0);
#endif
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < n_passes; ++p) {
        const TilePass &ps = passes[p];
        // the groups of the pass: their index bits with zeros inserted at the pass's four tile bits
        for (uint32_t grp = threadIdx.x; grp < (1u << (TILE_SEQ_BITS - 4)); grp += TILE_SEQ_THREADS) {
            uint32_t g0 = grp;
#pragma unroll
            for (int j = 0; j < 4; ++j) g0 = static_cast<uint32_t>(insert_zero(g0, ps.q[j]));
            amp_t x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c)
                x[c] = tile[g0 | ((c & 1) << ps.q[0]) | (((c >> 1) & 1) << ps.q[1]) | (((c >> 2) & 1) << ps.q[2]) | (((c >> 3) & 1) << ps.q[3])];
            seq_run16(x, gates + ps.first, ps.count);
#pragma unroll
            for (int c = 0; c < 16; ++c)
                tile[g0 | ((c & 1) << ps.q[0]) | (((c >> 1) & 1) << ps.q[1]) | (((c >> 2) & 1) << ps.q[2]) | (((c >> 3) & 1) << ps.q[3])] = x[c];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) st<NT>(a + base + off[q * RPW + i], tile[(q * RPW + i) * 64 + lane]);
}

// A fused 5-qubit block as the sequence of its source gates (k_seq_big / k_seq_lds).  bits[j] = bit position of block leg j;
// gate g acts on block legs legs[2 g] (and legs[2 g + 1] when arity[g] == 2), its matrix follows the previous gate's in
// `mats` (8 or 32 doubles).  QSV_UNHANDLED_KQ: the register or the sequence does not fit this form (the caller applies
// the block's product matrix instead).
int qsvk_sequence5(qsv_state *st, const int *bits, int n_gates, const int *arity, const int *legs, const double *mats) {
    const int k = 5, D = 32;
    if (n_gates < 1 || n_gates > SEQ_MAX_GATES || st->n < k) return QSV_UNHANDLED_KQ;
    // multiply-adds per 32 amplitudes: 256 per one-qubit gate, 512 per two-qubit gate, 4096 for the dense block
    int work = 0;
    for (int gi = 0; gi < n_gates; ++gi) work += arity[gi] == 1 ? 256 : 512;
    if (work > (st->sequence_work >= 0 ? st->sequence_work : seq_max_work())) return QSV_UNHANDLED_KQ;
    const uint64_t W = st->amps >> k;
    if (W < 64 || W % 64) return QSV_UNHANDLED_KQ;
    // register index c = (h << KL) | t: h bit i <-> high[i], t bit j <-> low[j] (as launch_dense_big's line-granular form)
    const Split s = split_targets(k, bits, st->n);
    if (!s.enough) return QSV_UNHANDLED_KQ;
    const std::vector<int> kb = kernel_bits(s);
    auto reg_bit = [&](int leg) { return static_cast<int>(std::find(kb.begin(), kb.end(), bits[leg]) - kb.begin()); };
    std::vector<SeqGate> rec(n_gates);
    const double *m = mats;
    for (int gi = 0; gi < n_gates; ++gi) {
        const int l0 = legs[2 * gi], l1 = legs[2 * gi + 1];
        if (arity[gi] == 1) {
            if (l0 < 0 || l0 >= k) return qsv_fail(QSV_EINVAL, "gate sequence: leg outside the block");
            rec[gi] = seq_record(1, reg_bit(l0), 0, m);
        } else if (arity[gi] == 2) {
            if (l0 < 0 || l0 >= k || l1 < 0 || l1 >= k || l0 == l1) return qsv_fail(QSV_EINVAL, "gate sequence: legs outside the block");
            rec[gi] = seq_record(2, reg_bit(l0), reg_bit(l1), m);
        } else {
            return QSV_UNHANDLED_KQ;
        }
        m += arity[gi] == 1 ? 8 : 32;
    }
    const std::vector<uint64_t> off = offsets(address_bits(s, true));
    StageRef staged;
    int rc = qsvk_stage(st, rec.data(), sizeof(SeqGate) * rec.size(), off.data(), sizeof(uint64_t) * D, &staged);
    if (rc) return rc;
    const SeqGate *dev_g = reinterpret_cast<const SeqGate *>(staged.dev);
    const uint64_t *dev_off = reinterpret_cast<const uint64_t *>(staged.dev + qsv_pad16(sizeof(SeqGate) * rec.size()));
    const bool nt = st->nontemporal != 0;
    const Enumeration e = enumeration(W, inserted_bits(s));
    if (s.low.empty()) {
        BigArgs g = with_enumeration<BigArgs>(e);
        g.regions = regions_or(st, 8);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_seq_big<%s>", nt ? "true" : "false");
        rc = launch_ranges(g, DISPATCH_ITEMS, [&](uint64_t items) {
            const dim3 gd(grid_for(items, QSV_BLOCK, 0)), bd(QSV_BLOCK);
            with_bool(nt, [&](auto NT) { hipLaunchKernelGGL(k_seq_big<NT.value>, gd, bd, 0, st->stream, st->data, g, dev_g, n_gates, dev_off); });
        });
    } else {
        LdsArgs g = with_enumeration<LdsArgs>(e);
        set_low_fields(g, low_fields(s));
        g.regions = regions_or(st, 8);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_seq_lds<%d, %s>", s.KB, nt ? "true" : "false");
        rc = launch_ranges(g, DISPATCH_ITEMS, [&](uint64_t items) {
            const dim3 gd(grid_for(items, QSV_BLOCK, 0)), bd(QSV_BLOCK);
            with_int<0, 3>(s.KB, [&](auto B) { with_bool(nt, [&](auto NT) {
                hipLaunchKernelGGL((k_seq_lds<B.value, NT.value>), gd, bd, 0, st->stream, st->data, g, dev_g, n_gates, dev_off);
            }); });
        });
    }
    return rc ? rc : qsvk_stage_done(st, staged);
}

// A fused block of k = 1..6 qubits as the list of its source gates on LDS tiles (k_seq_tile).  Arguments as
// qsvk_sequence5.  QSV_UNHANDLED_KQ: the register is too small for a tile, a gate acts on more than two qubits, or the
// list needs more passes than the kernel's table holds.
int qsvk_sequence_tile(qsv_state *st, int k, const int *bits, int n_gates, const int *arity, const int *legs,
                       const double *mats) {
    if (k < 1 || k > 6 || n_gates < 1 || n_gates > SEQ_MAX_GATES || st->n < TILE_SEQ_BITS) return QSV_UNHANDLED_KQ;
    const TileCut cut = cut_tile_passes(st->n, k, bits, n_gates, arity, legs, mats);
    if (cut.status == TileCut::UNHANDLED) return QSV_UNHANDLED_KQ;
    if (cut.status == TileCut::LEG_OUTSIDE) return qsv_fail(QSV_EINVAL, "gate sequence: leg outside the block");
    if (cut.status == TileCut::LEGS_EQUAL) return qsv_fail(QSV_EINVAL, "gate sequence: legs outside the block");
    const std::vector<int> &tile_bits = cut.tile_bits;
    const std::vector<uint64_t> off = offsets(std::vector<int>(tile_bits.begin() + 6, tile_bits.end()));   // [rows]
    // one image: [gates | passes | row offsets]
    const size_t gates_bytes = qsv_pad16(sizeof(SeqGate) * cut.rec.size()), passes_bytes = qsv_pad16(sizeof(TilePass) * cut.passes.size());
    std::vector<char> image(gates_bytes + passes_bytes, 0);
    std::memcpy(image.data(), cut.rec.data(), sizeof(SeqGate) * cut.rec.size());
    std::memcpy(image.data() + gates_bytes, cut.passes.data(), sizeof(TilePass) * cut.passes.size());
    StageRef staged;
    int rc = qsvk_stage(st, image.data(), image.size(), off.data(), sizeof(uint64_t) * off.size(), &staged);
    if (rc) return rc;
    const SeqGate *dev_g = reinterpret_cast<const SeqGate *>(staged.dev);
    const TilePass *dev_p = reinterpret_cast<const TilePass *>(staged.dev + gates_bytes);
    const uint64_t *dev_off = reinterpret_cast<const uint64_t *>(staged.dev + qsv_pad16(image.size()));
    TileSeqArgs ta;
    std::memset(&ta, 0, sizeof(ta));
    ta.g = with_enumeration<BigArgs>(enumeration(st->amps >> TILE_SEQ_BITS, tile_bits));   // tiles: the index with every tile bit taken out
    for (int j = 0; j < 6; ++j) ta.lane_bit[j] = static_cast<uint32_t>(tile_bits[j]);
    ta.g.regions = regions_or(st, 8);
    const bool nt = st->nontemporal != 0;
    const size_t lds = sizeof(amp_t) << TILE_SEQ_BITS;
    static bool raised = false;
    if (!raised) {
        QSV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_seq_tile<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)));
        QSV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_seq_tile<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)));
        raised = true;
    }
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_seq_tile<%s>", nt ? "true" : "false");
    const int n_passes = static_cast<int>(cut.passes.size());
    st->last_passes = n_passes;
    rc = launch_ranges(ta.g, DISPATCH_TILES, [&](uint64_t tiles) {
        const dim3 gd(static_cast<unsigned>(tiles)), bd(TILE_SEQ_THREADS);
        with_bool(nt, [&](auto NT) { hipLaunchKernelGGL(k_seq_tile<NT.value>, gd, bd, lds, st->stream, st->data, ta, dev_g, dev_p, n_passes, dev_off); });
    });
    return rc ? rc : qsvk_stage_done(st, staged);
}
