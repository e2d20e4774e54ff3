// The register's plumbing: the staging ring that carries gate matrices and tables to the device without a host-side
// wait (qsvk_stage, qsvk_stage_done, qsvk_ensure_matrix), the spare buffer of the out-of-place operations (qsvk_scratch,
// qsvk_adopt) and the register-to-register copy kernel (qsvk_copy).

#include "qsv_internal.h"
#include "qsv_device.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

namespace {

// Register-to-register copy (qsv_copy; also the "what does a plain copy reach on this box" leg of bench.py), every
// wave-instruction a whole 1 KiB segment, nontemporal both ways (hipMemcpy D2D: 4.9 TB/s).  Forms (QSV_COPY_MODE, for
// measurements; profiles/r03_copy_kernel.txt): 0 = four amplitudes per thread through registers, 1 = one amplitude per
// thread through registers, 2 = one per thread, HBM -> LDS directly (global_load_lds_dwordx4, as the gate kernels
// load) and LDS -> HBM.
constexpr int COPY_ITEMS = 4;
template <int MODE>
__global__ __launch_bounds__(QSV_BLOCK) void k_copy(amp_t *__restrict__ dst, const amp_t *__restrict__ src, uint32_t regions) {
    const uint64_t tile = (regions > 1 && gridDim.x % regions == 0)
                              ? (blockIdx.x % regions) * static_cast<uint64_t>(gridDim.x / regions) + blockIdx.x / regions
                              : blockIdx.x;
    if constexpr (MODE == 0) {
        const uint64_t base = tile * (QSV_BLOCK * COPY_ITEMS) + threadIdx.x;
        amp_t v[COPY_ITEMS];
#pragma unroll
        for (int u = 0; u < COPY_ITEMS; ++u) v[u] = __builtin_nontemporal_load(src + base + u * QSV_BLOCK);
#pragma unroll
        for (int u = 0; u < COPY_ITEMS; ++u) __builtin_nontemporal_store(v[u], dst + base + u * QSV_BLOCK);
    } else if constexpr (MODE == 1) {
        const uint64_t i = tile * QSV_BLOCK + threadIdx.x;
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
    } else {
        __shared__ amp_t lds[QSV_BLOCK];
        const uint64_t i = tile * QSV_BLOCK + threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
        __builtin_amdgcn_global_load_lds(src + i, lds + (threadIdx.x & ~63u), 16, 0, 2);
#endif
        __syncthreads();
        __builtin_nontemporal_store(lds[threadIdx.x], dst + i);
    }
}

}  // namespace

int qsvk_ensure_matrix(qsv_state *st, size_t bytes) {
    if (st->dev_matrix_bytes >= bytes) return QSV_OK;
    if (st->dev_matrix) {
        QSV_HIP(hipStreamSynchronize(st->stream));
        QSV_HIP(hipFree(st->dev_matrix));
        st->dev_matrix = nullptr;
        st->dev_matrix_bytes = 0;
    }
    if (hipMalloc(reinterpret_cast<void **>(&st->dev_matrix), bytes) != hipSuccess)
        return qsv_fail(QSV_ENOMEM, "device allocation of the gate-matrix buffer failed");
    st->dev_matrix_bytes = bytes;
    return QSV_OK;
}

// Gate matrices and index tables come from host memory that dies when the call returns.  Copying them to the device
// with hipMemcpyAsync + hipStreamSynchronize makes every such gate wait for the previous kernel before its own launch
// can even be queued: 72 us of idle GPU between the fused blocks of a circuit (4 % of the pass at n = 28, two thirds of
// it at n = 22).  Instead the data is copied into the next slot of a pinned ring by the CPU, a transfer to the slot's
// device mirror is queued on the register's stream in front of the kernel, and an event recorded behind the
// kernel says when the slot may be overwritten -- the host only ever waits when it is a whole ring ahead of the GPU.
// Payloads larger than a slot take the synchronous road through st->dev_matrix.
// The transfer itself is a small kernel that reads the pinned slot over PCIe (pinned host memory is mapped into the
// device's address space): a copy-engine transfer queued between two kernels starts ~45 us after the first kernel ends
// (the dependency crosses from the compute queue to the SDMA queue), a kernel behind a kernel on the same queue ~5 us.
__global__ __launch_bounds__(QSV_BLOCK) void k_stage_copy(uint4 *__restrict__ dst, const uint4 *__restrict__ src, uint32_t n16) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

int qsvk_stage(qsv_state *st, const void *a, size_t bytes_a, const void *b, size_t bytes_b, StageRef *out) {
    const size_t off_b = qsv_pad16(bytes_a), total = off_b + bytes_b;
    if (total > QSV_STAGE_BYTES) {
        const int rc = qsvk_ensure_matrix(st, total);
        if (rc) return rc;
        char *dev = reinterpret_cast<char *>(st->dev_matrix);
        if (bytes_a) QSV_HIP(hipMemcpyAsync(dev, a, bytes_a, hipMemcpyHostToDevice, st->stream));
        if (bytes_b) QSV_HIP(hipMemcpyAsync(dev + off_b, b, bytes_b, hipMemcpyHostToDevice, st->stream));
        QSV_HIP(hipStreamSynchronize(st->stream));  // the sources are pageable host memory that dies at return
        out->dev = dev;
        out->slot = -1;
        return QSV_OK;
    }
    if (!st->stage_dev) {
        // events first, then the buffers; stage_dev is published last, so a failure half way leaves the ring absent
        // (not half built) and the next call starts over
        hipEvent_t events[QSV_STAGE_SLOTS] = {};
        for (int i = 0; i < QSV_STAGE_SLOTS; ++i)
            if (hipEventCreate(&events[i]) != hipSuccess) {
                for (int j = 0; j < i; ++j) (void)hipEventDestroy(events[j]);
                return qsv_fail(QSV_EHIP, "event creation for the gate-matrix staging ring failed");
            }
        char *host = nullptr, *dev = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&host), QSV_STAGE_SLOTS * QSV_STAGE_BYTES, 0) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&dev), QSV_STAGE_SLOTS * QSV_STAGE_BYTES) != hipSuccess) {
            if (host) (void)hipHostFree(host);
            for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
            return qsv_fail(QSV_ENOMEM, "allocation of the gate-matrix staging ring failed");
        }
        for (int i = 0; i < QSV_STAGE_SLOTS; ++i) st->stage_done[i] = events[i];
        st->stage_host = host;
        st->stage_dev = dev;
    }
    const int slot = static_cast<int>(st->stage_next++ % QSV_STAGE_SLOTS);
    if (st->stage_busy[slot]) {
        QSV_HIP(hipEventSynchronize(st->stage_done[slot]));
        st->stage_busy[slot] = false;
    }
    char *host = st->stage_host + slot * QSV_STAGE_BYTES, *dev = st->stage_dev + slot * QSV_STAGE_BYTES;
    if (bytes_a) std::memcpy(host, a, bytes_a);
    if (bytes_b) std::memcpy(host + off_b, b, bytes_b);
    const uint32_t n16 = static_cast<uint32_t>((total + 15) / 16);
    hipLaunchKernelGGL(k_stage_copy, dim3((n16 + QSV_BLOCK - 1) / QSV_BLOCK < 16 ? (n16 + QSV_BLOCK - 1) / QSV_BLOCK : 16), dim3(QSV_BLOCK), 0,
                       st->stream, reinterpret_cast<uint4 *>(dev), reinterpret_cast<const uint4 *>(host), n16);
    QSV_HIP(hipGetLastError());
    // the slot is protected from here on: whatever the caller does next (its launch may fail, it may return early), the
    // pinned slot is not rewritten before this copy kernel has read it.  qsvk_stage_done moves the mark behind the consumer.
    QSV_HIP(hipEventRecord(st->stage_done[slot], st->stream));
    st->stage_busy[slot] = true;
    out->dev = dev;
    out->slot = slot;
    return QSV_OK;
}

int qsvk_stage_done(qsv_state *st, const StageRef &ref) {
    if (ref.slot < 0) return QSV_OK;
    QSV_HIP(hipEventRecord(st->stage_done[ref.slot], st->stream));   // re-record: now behind the kernel that reads the slot
    st->stage_busy[ref.slot] = true;
    return QSV_OK;
}

// Out-of-place operations (measure, insert, permute, the mode contractions) write into the state's spare
// buffer and then swap it in (qsvk_adopt).  The spare is kept between calls: a circuit that alternates such
// operations ping-pongs between two allocations instead of paying hipMalloc/hipFree of the register per gate
// (measured: ~0.44 s per gate on a 16 GiB register).
int qsvk_scratch(qsv_state *st, uint64_t amps, amp_t **out) {
    if (amps == 0) amps = 1;
    if (st->spare_capacity < amps) {
        if (st->spare) {
            QSV_HIP(hipStreamSynchronize(st->stream));
            QSV_HIP(hipFree(st->spare));
            st->spare = nullptr;
            st->spare_capacity = 0;
        }
        if (hipMalloc(reinterpret_cast<void **>(&st->spare), sizeof(amp_t) * amps) != hipSuccess)
            return qsv_fail(QSV_ENOMEM, "device allocation of the spare register failed");
        st->spare_capacity = amps;
    }
    *out = st->spare;
    return QSV_OK;
}

// The spare buffer now holds the register (new_amps amplitudes): swap it in when the library owns the memory,
// copy it back when the caller does (a view's pointer must stay valid).
int qsvk_adopt(qsv_state *st, uint64_t new_amps) {
    if (st->owns_data) {
        std::swap(st->data, st->spare);
        std::swap(st->capacity, st->spare_capacity);
    } else {
        QSV_HIP(hipMemcpyAsync(st->data, st->spare, sizeof(amp_t) * new_amps, hipMemcpyDeviceToDevice, st->stream));
    }
    st->amps = new_amps;
    return QSV_OK;
}

int qsvk_copy(amp_t *dst, const amp_t *src, uint64_t amps, hipStream_t stream) {
    static const int mode = [] { const char *e = getenv("QSV_COPY_MODE"); return e ? atoi(e) : 1; }();
    static const int regions = [] { const char *e = getenv("QSV_COPY_REGIONS"); return e ? atoi(e) : 0; }();
    const uint64_t per_block = mode == 0 ? QSV_BLOCK * COPY_ITEMS : QSV_BLOCK;
    const uint64_t bulk = amps / per_block * per_block;
    for (uint64_t done = 0; done < bulk;) {   // an AQL dispatch counts work-items in 32 bits
        const uint64_t blocks = std::min<uint64_t>((bulk - done) / per_block, 1ull << 23);
        const dim3 gd(static_cast<unsigned>(blocks)), bd(QSV_BLOCK);
        with_int<0, 2>(mode, [&](auto MODE) { hipLaunchKernelGGL(k_copy<MODE.value>, gd, bd, 0, stream, dst + done, src + done, regions); });
        done += blocks * per_block;
    }
    if (bulk < amps) {
        hipError_t e = hipMemcpyAsync(dst + bulk, src + bulk, sizeof(amp_t) * (amps - bulk), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return qsv_fail(QSV_EHIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    }
    return check_launch();
}
