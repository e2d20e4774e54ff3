// Reversible register arithmetic on a qubit register (gfx950, wave64): modular addition and
// multiplication, register-controlled versions of both, xor lookups and value permutations, each ONE gather pass from the
// register into its spare buffer.  qsv_arith is the handle (both parameter sets and their tables on the device);
// qsvk_arith is the launcher behind qsv_apply_arith (qsv_api.hip).  Segments, forms, launch shapes, the reduction and the
// validation are qsv_arith_layout.h, and so is arith_source(), the whole index computation of the kernel.
//
// k_arith.  A work item is one setting of every index bit except the lane's item bits (spectators at or above bit 6): the
// lane evaluates the map once, then moves 2^ITEMS_LOG2 amplitudes that differ in the item bits only (one by default: the
// fastest measured).  The stores of a wave are 64 consecutive amplitudes per item; the loads differ from them in target bits
// alone, so with the lowest target, source and control bit at 3 or above they are whole 128-byte lines too.  Loads and stores are non-temporal as in k_permute_s: every amplitude is
// touched once.  The tables (32-bit words) are read with ordinary loads and stay in the caches.  All loads of a lane are
// issued before its first store.  The grid strides over the work items with 64-bit indices: grid x block stays below 2^28
// whatever the register's size.

#include "qsv_device.h"
#include "qsv_arith_layout.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace qsv_arith_layout;

static_assert(ARITH_BLOCK == QSV_BLOCK && ARITH_LANE_BITS == QSV_LANE_BITS && ARITH_STREAM_QUBITS == qsv_readout_layout::RO_MIN_QUBITS &&
              ARITH_INVERSE == QSV_ARITH_INVERSE, "qsv_arith_layout.h mirrors qsv_internal.h and qsv.h");
static_assert(KIND_ADD == QSV_ARITH_ADD && KIND_MUL == QSV_ARITH_MUL && KIND_ADD_REG == QSV_ARITH_ADD_REG && KIND_MUL_POW == QSV_ARITH_MUL_POW &&
              KIND_XOR_LOOKUP == QSV_ARITH_XOR_LOOKUP && KIND_PERMUTE == QSV_ARITH_PERMUTE, "the header's kinds are the layout's");

struct qsv_arith {
    int device = 0;
    Params p;
    uint32_t *dev_fwd = nullptr;     // table of p.gather_fwd on the device (nullptr: none)
    uint32_t *dev_inv = nullptr;     // table of p.gather_inv; == dev_fwd where the two tables are the same (XOR_LOOKUP)
};

namespace {

template <int BODY, bool POW2, int ITEMS_LOG2>
__global__ __launch_bounds__(QSV_BLOCK) void k_arith(const amp_t *__restrict__ src, amp_t *__restrict__ dst, const ArithArgs g,
                                                     const uint32_t *__restrict__ table) {
    constexpr int ITEMS = 1 << ITEMS_LOG2;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; w < g.W; w += stride) {
        const uint64_t to = arith_base(w, g);
        const uint64_t from = arith_source<BODY, POW2>(to, g, table);
        uint64_t off[ITEMS];
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) {
            off[u] = 0;
#pragma unroll
            for (int k = 0; k < ITEMS_LOG2; ++k)
                if ((u >> k) & 1) off[u] |= 1ull << g.item_bit[k];
        }
        amp_t v[ITEMS];
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) v[u] = __builtin_nontemporal_load(src + (from | off[u]));
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) __builtin_nontemporal_store(v[u], dst + (to | off[u]));
    }
}

// amplitudes per lane: one (qsv_arith_layout.h); QSV_ARITH_ITEMS = 0 / 1 / 2 caps them at 1 / 2 / 4 for measurements
int max_items_log2() {
    static const int v = [] {
        const char *e = getenv("QSV_ARITH_ITEMS");
        const int x = e ? atoi(e) : ARITH_DEFAULT_ITEMS_LOG2;
        return x >= 0 && x <= ARITH_MAX_ITEMS_LOG2 ? x : ARITH_DEFAULT_ITEMS_LOG2;
    }();
    return v;
}

template <int BODY, bool POW2>
void launch_body(const Shape &shape, hipStream_t stream, const amp_t *src, amp_t *dst, const ArithArgs &g, const uint32_t *table) {
    const dim3 gd(shape.grid), bd(QSV_BLOCK);
    with_int<0, ARITH_MAX_ITEMS_LOG2>(shape.items_log2, [&](auto IT) {
        hipLaunchKernelGGL((k_arith<BODY, POW2, IT.value>), gd, bd, 0, stream, src, dst, g, table);
    });
}

int upload(const std::vector<uint32_t> &host, uint32_t **dev) {
    *dev = nullptr;
    if (host.empty()) return QSV_OK;
    const size_t bytes = sizeof(uint32_t) * host.size();
    if (hipMalloc(reinterpret_cast<void **>(dev), bytes) != hipSuccess) {
        *dev = nullptr;
        return qsv_fail(QSV_ENOMEM, "device allocation of the map's table failed");
    }
    QSV_HIP(hipMemcpy(*dev, host.data(), bytes, hipMemcpyHostToDevice));
    return QSV_OK;
}

}  // namespace

// tbits / sbits / cbits: index bits, validated by the caller (qsv_apply_arith).  *launches = kernel launches made.
int qsvk_arith(qsv_state *st, const qsv_arith *op, const int *tbits, const int *sbits, int n_controls, const int *cbits, bool inverse,
               uint64_t *launches) {
    *launches = 0;
    const Params &p = op->p;
    const Set &set = inverse ? p.gather_inv : p.gather_fwd;
    if (set.identity) return QSV_OK;
    const uint32_t *table = inverse ? op->dev_inv : op->dev_fwd;
    const uint64_t used = used_mask(p.m, tbits, p.mx, sbits, n_controls, cbits);
    const Shape shape = launch_shape(st->n, used, max_items_log2());
    const ArithArgs g = make_args(p, set, shape, tbits, sbits, n_controls, cbits);
    amp_t *fresh = nullptr;
    int rc = qsvk_scratch(st, st->amps, &fresh);
    if (rc) return rc;
    switch (set.body) {
        case BODY_SHIFT:
            if (p.pow2) launch_body<BODY_SHIFT, true>(shape, st->stream, st->data, fresh, g, table);
            else launch_body<BODY_SHIFT, false>(shape, st->stream, st->data, fresh, g, table);
            break;
        case BODY_MULT:
            if (p.pow2) launch_body<BODY_MULT, true>(shape, st->stream, st->data, fresh, g, table);
            else launch_body<BODY_MULT, false>(shape, st->stream, st->data, fresh, g, table);
            break;
        case BODY_XOR: launch_body<BODY_XOR, true>(shape, st->stream, st->data, fresh, g, table); break;
        default: launch_body<BODY_TABLE, true>(shape, st->stream, st->data, fresh, g, table); break;
    }
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_arith<%s, %s, %d> %s", body_name(set.body), p.pow2 ? "true" : "false",
             shape.items_log2, form_name(shape.form));
    rc = check_launch();
    if (rc) return rc;
    *launches = 1;
    return qsvk_adopt(st, st->amps);
}

int qsvk_arith_describe(const qsv_arith *op, int *device, int *m, int *mx) {
    *device = op->device, *m = op->p.m, *mx = op->p.mx;
    return QSV_OK;
}

extern "C" {

int qsv_arith_create(int kind, int m, int mx, uint64_t a, uint64_t c, uint64_t modulus, const uint64_t *table, uint64_t table_len,
                     int device, qsv_arith **out) {
    if (!out) return qsv_fail(QSV_EINVAL, "null pointer");
    *out = nullptr;
    Params p;
    const char *refused = make_params(kind, m, mx, a, c, modulus, table, table_len, &p);
    if (refused) return qsv_fail(QSV_EINVAL, std::string("register map: ") + refused);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return qsv_fail(QSV_EHIP, "no HIP device");
    if (device < 0 || device >= count) return qsv_fail(QSV_EINVAL, "no such device");
    QSV_HIP(hipSetDevice(device));
    qsv_arith *op = new qsv_arith;
    op->device = device;
    op->p = std::move(p);
    int rc = upload(op->p.gather_fwd.table, &op->dev_fwd);
    if (rc == QSV_OK) {
        if (op->p.kind == KIND_XOR_LOOKUP) op->dev_inv = op->dev_fwd;
        else rc = upload(op->p.gather_inv.table, &op->dev_inv);
    }
    if (rc) {
        qsv_arith_destroy(op);
        return rc;
    }
    *out = op;
    return QSV_OK;
}

int qsv_arith_destroy(qsv_arith *op) {
    if (!op) return QSV_OK;
    (void)hipSetDevice(op->device);
    (void)hipDeviceSynchronize();      // kernels of any register's stream may still read the tables
    if (op->dev_inv && op->dev_inv != op->dev_fwd) (void)hipFree(op->dev_inv);
    if (op->dev_fwd) (void)hipFree(op->dev_fwd);
    delete op;
    return QSV_OK;
}

int qsv_arith_info(const qsv_arith *op, int *kind, int *m, int *mx) {
    if (!op) return qsv_fail(QSV_EINVAL, "null register map");
    if (kind) *kind = op->p.kind;
    if (m) *m = op->p.m;
    if (mx) *mx = op->p.mx;
    return QSV_OK;
}

}  // extern "C"
