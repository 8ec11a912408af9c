// framesum C ABI (include/framesum.h) -- context lifecycle, the device-resident and host-staged
// digest and fill calls, fs_digest_batch_multi, the setters and the test library's hooks; and the
// definitions of what framesum_ctx.h shares with the TX frame build (framesum_api_tx.cpp) and the RX
// coalesce (framesum_api_rx.cpp). No CPU fallback: every digest is computed by the gfx950 kernel
// (framesum_kernel.hip); a missing/unsupported device is an error.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "framesum_ctx.h"

using framesum::FsTables;
using namespace framesum::host;

// At least `bytes` + 256 bytes. A buffer in use by queued work is safe to regrow without a wait of
// its own: hipFree synchronizes the device before it releases the memory (only a staging slot waits
// first, for its `consumed` event: ensure_slot).
fs_status DevBuf::grow(fs_ctx* ctx, uint64_t bytes, const char* what) {
    if (bytes <= cap) return FS_SUCCESS;
    release();
    if (hipMalloc(&p, bytes + 256) != hipSuccess) return set_err(ctx, FS_E_NOMEM, what);
    cap = bytes + 256;
    return FS_SUCCESS;
}

void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

namespace framesum {
namespace host {

thread_local std::string g_create_err;

fs_status set_err(fs_ctx* ctx, fs_status code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else g_create_err = msg;
    return code;
}

fs_status hip_err(fs_ctx* ctx, hipError_t e, const char* what) {
    return set_err(ctx, FS_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

fs_status ensure_slot(fs_ctx* ctx, HostSlot& sl, uint64_t frame_bytes, uint32_t n) {
    const auto grow = [&](DevBuf& b, uint64_t bytes, const char* what) -> fs_status {
        if (bytes > b.cap && sl.used) FS_HIP(ctx, hipEventSynchronize(sl.consumed));
        return b.grow(ctx, bytes, what);
    };
    const char* const desc = "hipMalloc descriptor staging";
    fs_status st = grow(sl.frames, frame_bytes, "hipMalloc frames staging");
    if (st == FS_SUCCESS) st = grow(sl.offsets, (uint64_t)n * 8, desc);
    if (st == FS_SUCCESS) st = grow(sl.lengths, (uint64_t)n * 4, desc);
    if (st == FS_SUCCESS) st = grow(sl.out, (uint64_t)n * (sizeof(fs_digest) + 1), desc);
    if (st == FS_SUCCESS) st = grow(sl.status, n, desc);
    return st;
}

fs_status begin_host_call(fs_ctx* ctx) {
    FS_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->host_dirty) return FS_SUCCESS;
    FS_HIP(ctx, hipStreamSynchronize(ctx->compute_stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->copy_stream2));
    ctx->host_dirty = false;
    return FS_SUCCESS;
}

void drain_host_streams(fs_ctx* ctx) {
    const bool ok = hipStreamSynchronize(ctx->compute_stream) == hipSuccess &&
                    hipStreamSynchronize(ctx->copy_stream) == hipSuccess &&
                    hipStreamSynchronize(ctx->copy_stream2) == hipSuccess;
    if (ok) ctx->host_dirty = false;
}

hipError_t launch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                  uint32_t mtu, fs_digest* out, uint8_t* status, hipStream_t stream, FsOp op, uint8_t* wframes,
                  uint32_t tx, int force) {
    const int wgs = ctx->workgroups > 0 && ctx->workgroups < ctx->num_cus ? ctx->workgroups : ctx->num_cus;
    return launch_digest(frames, offsets, lengths, n, mtu, ctx->d_tables, out, status, stream, wgs, ctx->choice,
                         ctx->h_report, ctx->d_report, force >= 0 ? force : ctx->force_kernel, op, wframes, tx);
}

fs_status stage_batch(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, uint64_t lo, uint64_t hi,
                      const uint64_t* offsets, const uint32_t* lengths, uint32_t n, Staged& s) {
    uint64_t cpy_lo, cpy_hi;
    plan::copy_span(lo, hi, frames_bytes, cpy_lo, cpy_hi);
    HostSlot& sl = ctx->slot[0];
    const fs_status st = ensure_slot(ctx, sl, cpy_hi - cpy_lo + 64, n);
    if (st != FS_SUCCESS) return st;
    ctx->host_dirty = true;  // until this call has waited for all of its work
    const hipStream_t ks = ctx->compute_stream;
    if (sl.used) FS_HIP_DRAIN(ctx, hipStreamWaitEvent(ks, sl.consumed, 0));
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(sl.frames.p, frames + cpy_lo, cpy_hi - cpy_lo, hipMemcpyHostToDevice, ks));
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(sl.offsets.p, offsets, (size_t)n * 8, hipMemcpyHostToDevice, ks));
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(sl.lengths.p, lengths, (size_t)n * 4, hipMemcpyHostToDevice, ks));
    s = Staged{&sl, ks, reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(sl.frames.p) - cpy_lo),
               sl.offsets.as<uint64_t>(), sl.lengths.as<uint32_t>(), sl.out.as<fs_digest>(), sl.status.p};
    return FS_SUCCESS;
}

fs_status finish_staged(fs_ctx* ctx, const Staged& s) {
    FS_HIP_DRAIN(ctx, hipEventRecord(s.sl->consumed, s.ks));
    s.sl->used = true;
    FS_HIP_DRAIN(ctx, hipStreamSynchronize(s.ks));
    ctx->host_dirty = false;
    return FS_SUCCESS;
}

}  // namespace host
}  // namespace framesum

namespace {

// h_pin layout for n frames: offsets (8n) | lengths (4n) | digests (8n) | status (n)
fs_status ensure_pinned(fs_ctx* ctx, uint32_t n) {
    if (n <= ctx->cap_pin_n) return FS_SUCCESS;
    if (ctx->h_pin) FS_HIP(ctx, hipHostFree(ctx->h_pin));
    ctx->h_pin = nullptr;
    ctx->d_pin = nullptr;
    ctx->cap_pin_n = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&ctx->h_pin), (size_t)n * 21 + 64, hipHostMallocMapped) != hipSuccess)
        return set_err(ctx, FS_E_NOMEM, "hipHostMalloc descriptor mirror");
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_pin), ctx->h_pin, 0) != hipSuccess) {
        (void)hipHostFree(ctx->h_pin);
        ctx->h_pin = nullptr;
        return set_err(ctx, FS_E_HIP, "hipHostGetDevicePointer of the descriptor mirror");
    }
    ctx->cap_pin_n = n;
    return FS_SUCCESS;
}

// Wait on the host for `ev` by polling: HIP's blocking wait wakes the host about 25 us after the
// work ends, a third of a short host-staged call. After 2 ms of polling (a long
// batch) it falls back to the blocking wait instead of burning the core.
hipError_t host_wait(hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return hipEventSynchronize(ev);
    }
}

// Is [p, p + bytes) inside ONE page-locked host allocation the GPU can copy from / to asynchronously
// (fs_host_alloc, hipHostMalloc, hipHostRegister)? Then a host-staged call copies straight from / to
// it, or has the kernel read or write it in place, instead of going through the context's pinned
// mirror. The whole span is checked, not only its start: a DMA or a kernel access past the end of a
// pinned allocation would fault the GPU, where the mirror path's host memcpy stays on the host.
bool is_pinned(const void* p, size_t bytes) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory: not an error of the call
        return false;
    }
    if (a.type != hipMemoryTypeHost) return false;
    void* start = nullptr;
    size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, const_cast<void*>(p)) != hipSuccess ||
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return false;  // the span cannot be checked: take the mirror path
    }
    const uintptr_t b = reinterpret_cast<uintptr_t>(start), q = reinterpret_cast<uintptr_t>(p);
    return q >= b && bytes <= size && q - b <= size - bytes;
}

// The argument checks at the head of a batch entry point `fn` (`aligned`: the kernel reads `frames`
// itself, so they must be 4-byte aligned). An empty batch passes: the caller returns FS_SUCCESS.
fs_status check_batch(fs_ctx* ctx, const char* fn, const void* frames, const void* offsets, const void* lengths,
                      uint32_t n, const void* out, bool aligned) {
    if (n == 0) return FS_SUCCESS;
    if (n > kMaxFrames) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": n too large (at most 2^31 frames per call)");
    if (!frames || !offsets || !lengths || !out) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null pointer");
    if (aligned && (reinterpret_cast<uintptr_t>(frames) & 3u))
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": frames must be 4-byte aligned");
    return FS_SUCCESS;
}

// The device address of pinned host memory [p, p + bytes) the kernel can read or write directly, or
// null.
void* mapped(void* p, size_t bytes) {
    if (!p || !is_pinned(p, bytes)) return nullptr;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return d;
}

// Where the one launch of a host-staged call writes its n digests and verdicts: straight to host
// memory (mapped pinned memory: no D2H copy, no gap before it), into the caller's arrays when they
// are pinned, else into the context's pinned mirror (ensure_pinned), which copy_out delivers after
// the wait.
struct ResultTarget {
    fs_digest* d_out;
    uint8_t* d_st;
    bool direct;
};
ResultTarget result_target(const fs_ctx* ctx, fs_digest* out, uint8_t* status, uint32_t n) {
    void* d_out = mapped(out, (size_t)n * sizeof(fs_digest));
    void* d_st = status ? mapped(status, n) : nullptr;
    const bool direct = d_out && (!status || d_st);
    if (!direct) {
        d_out = ctx->d_pin + (size_t)n * 12;
        d_st = status ? ctx->d_pin + (size_t)n * 20 : nullptr;
    }
    return ResultTarget{static_cast<fs_digest*>(d_out), static_cast<uint8_t*>(d_st), direct};
}
void copy_out(const fs_ctx* ctx, const ResultTarget& t, fs_digest* out, uint8_t* status, uint32_t n) {
    if (t.direct) return;
    std::memcpy(out, ctx->h_pin + (size_t)n * 12, (size_t)n * sizeof(fs_digest));
    if (status) std::memcpy(status, ctx->h_pin + (size_t)n * 20, n);
}

}  // namespace

extern "C" {

uint32_t fs_abi_version(void) { return FRAMESUM_ABI_VERSION; }

int fs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

fs_status fs_ctx_create(int device, fs_ctx** out) {
    if (!out) return set_err(nullptr, FS_E_INVALID, "fs_ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return set_err(nullptr, FS_E_NODEVICE, "fs_ctx_create: no such HIP device");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return set_err(nullptr, FS_E_NODEVICE, "fs_ctx_create: hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(nullptr, FS_E_NODEVICE, std::string("fs_ctx_create: device is ") + prop.gcnArchName +
                                                   ", this build targets gfx950 only");
    fs_ctx* ctx = new (std::nothrow) fs_ctx();
    if (!ctx) return set_err(nullptr, FS_E_NOMEM, "fs_ctx_create: out of host memory");
    ctx->device = device;
    ctx->num_cus = prop.multiProcessorCount;
    hipError_t e = hipSetDevice(device);
    FsTables* h = new (std::nothrow) FsTables;
    if (e != hipSuccess || !h) {
        delete h;
        delete ctx;
        return set_err(nullptr, FS_E_HIP, "fs_ctx_create: hipSetDevice / table alloc failed");
    }
    framesum::build_tables(h);
    e = hipMalloc(&ctx->d_tables, sizeof(FsTables));
    if (e == hipSuccess) e = hipMemcpy(ctx->d_tables, h, sizeof(FsTables), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        void* hp = nullptr;
        e = hipHostMalloc(&hp, 64, hipHostMallocMapped);
        if (e == hipSuccess) {
            ctx->h_report = static_cast<volatile uint32_t*>(hp);
            for (int w = 0; w < 16; ++w) ctx->h_report[w] = 0u;
            e = hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_report), hp, 0);
        }
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->compute_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->copy_stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->desc_copied, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->host_done, hipEventDisableTiming);
    for (int k = 0; k < kHostSlots && e == hipSuccess; ++k) {
        e = hipEventCreateWithFlags(&ctx->slot[k].copied, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->slot[k].consumed, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->slot[k].landed, hipEventDisableTiming);
    }
    delete h;
    if (e != hipSuccess) {
        std::string msg = std::string("fs_ctx_create: ") + hipGetErrorString(e);
        fs_ctx_destroy(ctx);
        return set_err(nullptr, FS_E_HIP, msg);
    }
    *out = ctx;
    return FS_SUCCESS;
}

fs_status fs_ctx_destroy(fs_ctx* ctx) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    (void)hipSetDevice(ctx->device);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->compute_stream) (void)hipStreamSynchronize(ctx->compute_stream);
    if (ctx->copy_stream2) (void)hipStreamSynchronize(ctx->copy_stream2);
    if (ctx->copy_stream2) (void)hipStreamDestroy(ctx->copy_stream2);
    if (ctx->desc_copied) (void)hipEventDestroy(ctx->desc_copied);
    if (ctx->host_done) (void)hipEventDestroy(ctx->host_done);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->compute_stream) (void)hipStreamDestroy(ctx->compute_stream);
    for (HostSlot& sl : ctx->slot) {
        if (sl.copied) (void)hipEventDestroy(sl.copied);
        if (sl.consumed) (void)hipEventDestroy(sl.consumed);
        if (sl.landed) (void)hipEventDestroy(sl.landed);
    }
    for (SegStage& sg : ctx->seg_stage) {
        if (sg.done) (void)hipEventSynchronize(sg.done);
        if (sg.done) (void)hipEventDestroy(sg.done);
        if (sg.h) (void)hipHostFree(sg.h);
        (void)hipFree(sg.d);
    }
    (void)hipFree(ctx->d_seg_tables);
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    if (ctx->h_report) (void)hipHostFree(const_cast<uint32_t*>(ctx->h_report));
    (void)hipFree(ctx->d_tables);
    delete ctx;  // (every DevBuf of the context and its slots frees itself here)
    return FS_SUCCESS;
}

const char* fs_last_error(const fs_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

// The three device-resident calls: one launch of `op` on the caller's stream. `wframes`: the frames
// as the TX fill writes them (null otherwise), `flags` its FS_FILL_* flags (0 otherwise).
static fs_status digest_resident(fs_ctx* ctx, const char* fn, framesum::FsOp op, const uint8_t* frames, uint8_t* wframes,
                                 uint32_t flags, const uint64_t* offsets, const uint32_t* lengths, uint32_t n, uint32_t mtu,
                                 fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (flags & ~(uint32_t)(FS_FILL_CSUM | FS_FCS_APPEND)) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": unknown flags");
    const fs_status st = check_batch(ctx, fn, frames, offsets, lengths, n, out, true);
    if (n == 0 || st != FS_SUCCESS) return st;
    FS_HIP(ctx, hipSetDevice(ctx->device));
    FS_HIP(ctx, launch(ctx, frames, offsets, lengths, n, mtu, out, status, reinterpret_cast<hipStream_t>(stream), op, wframes, flags));
    return FS_SUCCESS;
}

fs_status fs_digest_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                          uint32_t n, uint32_t mtu, fs_digest* out, uint8_t* status, void* stream) {
    return digest_resident(ctx, "fs_digest_batch", framesum::FsOp::kDigest, frames, nullptr, 0, offsets, lengths, n, mtu, out,
                           status, stream);
}

fs_status fs_fill_batch(fs_ctx* ctx, uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                        uint32_t mtu, uint32_t flags, fs_digest* out, uint8_t* status, void* stream) {
    return digest_resident(ctx, "fs_fill_batch", framesum::FsOp::kFill, frames, frames, flags, offsets, lengths, n, mtu, out,
                           status, stream);
}

fs_status fs_digest_batch_fcs(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                              uint32_t n, uint32_t mtu, fs_digest* out, uint8_t* status, void* stream) {
    return digest_resident(ctx, "fs_digest_batch_fcs", framesum::FsOp::kFcs, frames, nullptr, 0, offsets, lengths, n, mtu, out,
                           status, stream);
}

// The descriptor scan of a host-staged call, compiled for AVX-512 and AVX2 beside the baseline
// and picked at load time (its four min/max reductions vectorize: 65,536 descriptors in ~20 us
// instead of ~150 us on the baseline SSE2 build).
// (host code: hipcc also parses this file for the device, where multiversioning does not exist)
#if defined(__HIP_DEVICE_COMPILE__)
#define FS_HOST_CLONES
#else
#define FS_HOST_CLONES __attribute__((target_clones("arch=x86-64-v4", "arch=x86-64-v3", "default")))
#endif
FS_HOST_CLONES static framesum::plan::ScanCore scan_descriptors(const uint64_t* offsets, const uint32_t* lengths, uint32_t n) {
    return framesum::plan::scan_core(offsets, lengths, n);
}

// ... and the scan of a fs_digest_batch_host call, with the error set when a frame is out of range
// (sc.bad < n).
static framesum::plan::Scan scan_host(fs_ctx* ctx, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                                      uint64_t frames_bytes) {
    const framesum::plan::Scan sc =
        framesum::plan::scan_from(scan_descriptors(offsets, lengths, n), offsets, lengths, n, frames_bytes);
    if (sc.bad < n)
        set_err(ctx, FS_E_INVALID, "fs_digest_batch_host: frame " + std::to_string(sc.bad) + " ends past frames_bytes");
    return sc;
}

// A host-staged batch that fits one staging chunk (path 1). Everything runs on the compute stream,
// in its order: the descriptor copy (queued by the caller before its scan, straight from the
// caller's arrays when they are pinned), the frames' H2D copy into slot 0, one launch that writes the
// digests and verdicts into host memory through a mapped pointer (the caller's arrays when pinned,
// else the context's mirror, copied out after the wait; no D2H copy), then a polled wait.
static fs_status host_single(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                             const uint32_t* lengths, uint32_t n, uint32_t mtu, fs_digest* out, uint8_t* status,
                             const framesum::plan::Scan& sc, int force) {
    ctx->last_host_path = 1;
    uint64_t cpy_lo, cpy_hi;
    framesum::plan::copy_span(sc.lo, sc.hi, frames_bytes, cpy_lo, cpy_hi);
    HostSlot& sl = ctx->slot[0];
    fs_status st = ensure_slot(ctx, sl, cpy_hi - cpy_lo + 64, n);
    if (st != FS_SUCCESS) {
        // the descriptor copy already queued may still read the caller's arrays
        drain_host_streams(ctx);
        return st;
    }
    const ResultTarget rt = result_target(ctx, out, status, n);
    const hipStream_t ks = ctx->compute_stream;
    // the frames behind the descriptors (issued by the caller before the scan), then the kernel, in
    // the compute stream's order: no cross-stream event between them
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(sl.frames.p, frames + cpy_lo, cpy_hi - cpy_lo, hipMemcpyHostToDevice, ks));
    if (ctx->fault_chunk == 0) {
        drain_host_streams(ctx);
        return set_err(ctx, FS_E_NOMEM, "fs_digest_batch_host: injected failure (test hook)");
    }
    const uint8_t* base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(sl.frames.p) - cpy_lo);
    const uint64_t* d_off = ctx->desc.as<const uint64_t>();
    const uint32_t* d_len = ctx->desc.as<const uint32_t>((size_t)n * 8);
    FS_HIP_DRAIN(ctx, launch(ctx, base, d_off, d_len, n, mtu, rt.d_out, rt.d_st, ks, framesum::FsOp::kDigest, nullptr, 0,
                             force));
    FS_HIP_DRAIN(ctx, hipEventRecord(sl.consumed, ks));
    sl.used = true;
    FS_HIP_DRAIN(ctx, hipEventRecord(ctx->host_done, ks));
    FS_HIP_DRAIN(ctx, host_wait(ctx->host_done));
    copy_out(ctx, rt, out, status, n);
    ctx->host_dirty = false;
    return FS_SUCCESS;
}

// A host-staged batch read in place: frames, offsets and lengths in pinned host memory the device
// addresses directly (mapped), results written to host memory by the kernel (the caller's arrays when
// pinned, else the mirror). The small-frame kernel only: its lanes read whole 16-B chunks of adjacent
// frames, which the memory system turns into full-line PCIe reads.
static fs_status host_inplace(fs_ctx* ctx, const uint8_t* d_frames, const uint64_t* d_off, const uint32_t* d_len,
                              uint32_t n, uint32_t mtu, fs_digest* out, uint8_t* status) {
    ctx->last_host_path = 2;
    fs_status st = ensure_pinned(ctx, n);
    if (st != FS_SUCCESS) return st;
    const ResultTarget rt = result_target(ctx, out, status, n);
    ctx->host_dirty = true;
    const hipStream_t ks = ctx->compute_stream;
    FS_HIP_DRAIN(ctx, launch(ctx, d_frames, d_off, d_len, n, mtu, rt.d_out, rt.d_st, ks, framesum::FsOp::kDigest, nullptr,
                             0, framesum::kForceSmallExact));
    FS_HIP_DRAIN(ctx, hipEventRecord(ctx->host_done, ks));
    FS_HIP_DRAIN(ctx, host_wait(ctx->host_done));
    copy_out(ctx, rt, out, status, n);
    ctx->host_dirty = false;
    return FS_SUCCESS;
}

fs_status fs_digest_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                               const uint32_t* lengths, uint32_t n, uint32_t mtu, fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    const fs_status ast = check_batch(ctx, "fs_digest_batch_host", frames, offsets, lengths, n, out, false);
    if (n == 0 || ast != FS_SUCCESS) return ast;
    fs_status pst = begin_host_call(ctx);
    if (pst != FS_SUCCESS) return pst;
    if (n <= kChunkFrames && ctx->force_kernel != 2 && ctx->force_kernel != 3 && ctx->force_kernel != 4) {
        // A batch of short frames whose frames, offsets and lengths are all in pinned host memory:
        // the small-frame kernel reads them in place over PCIe and writes its results to host
        // memory, so the call is one launch -- no copies, no gaps between DMA commands.
        // (the frames' span is checked once the scan has found it: the 16-B chunks the kernel reads
        // stay in the pages that hold frame bytes, and pinned allocations are whole pages)
        const void* dof = mapped(const_cast<uint64_t*>(offsets), (size_t)n * 8);
        const void* dln = dof ? mapped(const_cast<uint32_t*>(lengths), (size_t)n * 4) : nullptr;
        if (dln && is_pinned(frames, 1)) {
            const framesum::plan::Scan sc = scan_host(ctx, offsets, lengths, n, frames_bytes);
            if (sc.bad < n) return FS_E_INVALID;
            const void* df = sc.hi > sc.lo ? mapped(const_cast<uint8_t*>(frames + sc.lo), sc.hi - sc.lo) : nullptr;
            if (df && framesum::host_force(ctx->force_kernel, sc.max_len, sc.min_len) == framesum::kForceSmallExact &&
                (reinterpret_cast<uintptr_t>(frames) & 3u) == 0u)
                return host_inplace(ctx, static_cast<const uint8_t*>(df) - sc.lo, static_cast<const uint64_t*>(dof),
                                    static_cast<const uint32_t*>(dln), n, mtu, out, status);
        }
    }
    if (n <= kChunkFrames) {
        // The descriptors go to the device first, while the host scans them (they are n elements
        // of the caller's arrays whatever the scan finds; a frame out of range fails the call before
        // any frame byte is copied): straight from the caller's arrays when they are pinned (one
        // copy when the lengths follow the offsets, as the Go binding stages them), else through
        // the pinned mirror.
        pst = ctx->desc.grow(ctx, (uint64_t)n * 12, "hipMalloc descriptors");
        if (pst == FS_SUCCESS) pst = ensure_pinned(ctx, n);
        if (pst != FS_SUCCESS) return pst;
        ctx->host_dirty = true;  // until this call has waited for all of its work
        const bool pin_desc = is_pinned(offsets, (size_t)n * 8) && is_pinned(lengths, (size_t)n * 4);
        const uint64_t* src_off = offsets;
        const uint32_t* src_len = lengths;
        if (!pin_desc) {
            src_off = reinterpret_cast<const uint64_t*>(ctx->h_pin);
            src_len = reinterpret_cast<const uint32_t*>(ctx->h_pin + (size_t)n * 8);
            std::memcpy(ctx->h_pin, offsets, (size_t)n * 8);
            std::memcpy(ctx->h_pin + (size_t)n * 8, lengths, (size_t)n * 4);
        }
        const hipStream_t ks = ctx->compute_stream;
        if (reinterpret_cast<const uint8_t*>(src_off) + (size_t)n * 8 == reinterpret_cast<const uint8_t*>(src_len)) {
            FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->desc.p, src_off, (size_t)n * 12, hipMemcpyHostToDevice, ks));
        } else {
            FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->desc.p, src_off, (size_t)n * 8, hipMemcpyHostToDevice, ks));
            FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->desc.p + (size_t)n * 8, src_len, (size_t)n * 4, hipMemcpyHostToDevice, ks));
        }
        const framesum::plan::Scan sc = scan_host(ctx, offsets, lengths, n, frames_bytes);
        if (sc.bad < n) {
            drain_host_streams(ctx);  // the descriptor copy reads the caller's arrays: done before returning
            return FS_E_INVALID;
        }
        const int force = framesum::host_force(ctx->force_kernel, sc.max_len, sc.min_len);
        if (sc.hi - sc.lo <= kChunkBytes)
            return host_single(ctx, frames, frames_bytes, offsets, lengths, n, mtu, out, status, sc, force);
        FS_HIP(ctx, hipStreamSynchronize(ks));  // (the chunked path below stages the descriptors itself)
    }
    const framesum::plan::Scan sc = scan_host(ctx, offsets, lengths, n, frames_bytes);
    if (sc.bad < n) return FS_E_INVALID;
    const int force = framesum::host_force(ctx->force_kernel, sc.max_len, sc.min_len);
    ctx->host_dirty = true;  // until this call has waited for all of its work
    ctx->last_host_path = 3;
    pst = ensure_pinned(ctx, n);
    if (pst != FS_SUCCESS) return pst;
    pst = ctx->desc.grow(ctx, (uint64_t)n * 12, "hipMalloc descriptors");
    if (pst != FS_SUCCESS) return pst;
    uint64_t* h_off = reinterpret_cast<uint64_t*>(ctx->h_pin);
    uint32_t* h_len = reinterpret_cast<uint32_t*>(ctx->h_pin + (size_t)n * 8);
    fs_digest* h_out = reinterpret_cast<fs_digest*>(ctx->h_pin + (size_t)n * 12);
    uint8_t* h_st = ctx->h_pin + (size_t)n * 20;
    std::vector<framesum::plan::Chunk> chunks;
    try {
        framesum::plan::host_chunks(offsets, lengths, n, frames_bytes, kChunkBytes, kChunkFrames, chunks);
    } catch (const std::bad_alloc&) {
        return set_err(ctx, FS_E_NOMEM, "fs_digest_batch_host: out of host memory");
    }
    const hipStream_t ks = ctx->compute_stream;
    // chunk k's frame bytes into its slot, on copy stream k & 1 (once the slot's previous chunk
    // has been consumed by its kernel)
    auto copy_chunk = [&](size_t k) -> fs_status {
        const framesum::plan::Chunk& c = chunks[k];
        HostSlot& sl = ctx->slot[k % kHostSlots];
        fs_status st = ensure_slot(ctx, sl, c.cpy_hi - c.cpy_lo + 64, c.c1 - c.c0);
        if (st != FS_SUCCESS) return st;
        const hipStream_t cs = (k & 1u) ? ctx->copy_stream2 : ctx->copy_stream;
        if (sl.used) FS_HIP(ctx, hipStreamWaitEvent(cs, sl.consumed, 0));  // chunk k - kHostSlots done with it
        FS_HIP(ctx, hipMemcpyAsync(sl.frames.p, frames + c.cpy_lo, c.cpy_hi - c.cpy_lo, hipMemcpyHostToDevice, cs));
        FS_HIP(ctx, hipEventRecord(sl.copied, cs));
        return FS_SUCCESS;
    };
    // chunk k's results from the pinned mirror into the caller's arrays, once they have landed
    auto deliver = [&](size_t k) -> fs_status {
        const framesum::plan::Chunk& c = chunks[k];
        FS_HIP(ctx, host_wait(ctx->slot[k % kHostSlots].landed));
        std::memcpy(out + c.c0, h_out + c.c0, (size_t)(c.c1 - c.c0) * sizeof(fs_digest));
        if (status) std::memcpy(status + c.c0, h_st + c.c0, c.c1 - c.c0);
        return FS_SUCCESS;
    };
    // the first chunk's frames stream while the descriptors are mirrored (pinned) and then
    // copied, all of them in one copy (h_off and h_len are contiguous in the mirror)
    fs_status st = copy_chunk(0);
    if (st != FS_SUCCESS) return st;
    std::memcpy(h_off, offsets, (size_t)n * 8);
    std::memcpy(h_len, lengths, (size_t)n * 4);
    const uint64_t* d_off = ctx->desc.as<const uint64_t>();
    const uint32_t* d_len = ctx->desc.as<const uint32_t>((size_t)n * 8);
    FS_HIP(ctx, hipMemcpyAsync(ctx->desc.p, h_off, (size_t)n * 12, hipMemcpyHostToDevice, ctx->copy_stream2));
    FS_HIP(ctx, hipEventRecord(ctx->desc_copied, ctx->copy_stream2));
    FS_HIP(ctx, hipStreamWaitEvent(ks, ctx->desc_copied, 0));
    for (size_t chunk = 0; chunk < chunks.size(); ++chunk) {
        const uint32_t c0 = chunks[chunk].c0, c1 = chunks[chunk].c1;
        const uint64_t cpy_lo = chunks[chunk].cpy_lo;
        HostSlot& sl = ctx->slot[chunk % kHostSlots];
        const uint32_t cnt = c1 - c0;
        if (chunk > 0) {
            st = copy_chunk(chunk);
            if (st != FS_SUCCESS) return st;
        }
        if ((long)chunk == ctx->fault_chunk)
            return set_err(ctx, FS_E_NOMEM, "fs_digest_batch_host: injected failure (test hook)");
        FS_HIP(ctx, hipStreamWaitEvent(ks, sl.copied, 0));
        // the kernel addresses frame i at base + offsets[i]: base = staging - cpy_lo (4-B aligned)
        const uint8_t* base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(sl.frames.p) - cpy_lo);
        FS_HIP(ctx, launch(ctx, base, d_off + c0, d_len + c0, cnt, mtu, sl.out.as<fs_digest>(), status ? sl.status.p : nullptr, ks,
                           framesum::FsOp::kDigest, nullptr, 0, force));
        FS_HIP(ctx, hipEventRecord(sl.consumed, ks));
        sl.used = true;
        FS_HIP(ctx, hipMemcpyAsync(h_out + c0, sl.out.p, (size_t)cnt * sizeof(fs_digest), hipMemcpyDeviceToHost, ks));
        if (status) FS_HIP(ctx, hipMemcpyAsync(h_st + c0, sl.status.p, cnt, hipMemcpyDeviceToHost, ks));
        FS_HIP(ctx, hipEventRecord(sl.landed, ks));
        // chunk - 2's results while this one streams (its slot's `landed` is re-recorded by chunk + 1)
        if (chunk >= 2) {
            st = deliver(chunk - 2);
            if (st != FS_SUCCESS) return st;
        }
    }
    for (size_t k = chunks.size() >= 2 ? chunks.size() - 2 : 0; k < chunks.size(); ++k) {
        st = deliver(k);
        if (st != FS_SUCCESS) return st;
    }
    FS_HIP(ctx, hipStreamSynchronize(ks));
    ctx->host_dirty = false;
    return FS_SUCCESS;
}

fs_status fs_fill_batch_host(fs_ctx* ctx, uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                             const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags, fs_digest* out,
                             uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (flags & ~(uint32_t)(FS_FILL_CSUM | FS_FCS_APPEND))
        return set_err(ctx, FS_E_INVALID, "fs_fill_batch_host: unknown flags");
    const fs_status ast = check_batch(ctx, "fs_fill_batch_host", frames, offsets, lengths, n, out, false);
    if (n == 0 || ast != FS_SUCCESS) return ast;
    // One staged span [lo, hi) (the frames and, with FS_FCS_APPEND, their FCS bytes), copied in,
    // filled, copied back. Not chunk-pipelined: written spans of unordered batches may interleave.
    const uint32_t extra = (flags & FS_FCS_APPEND) ? 4u : 0u;
    const framesum::plan::Scan sc = framesum::plan::scan_batch(offsets, lengths, n, frames_bytes, extra);
    if (sc.bad < n)
        return set_err(ctx, FS_E_INVALID, "fs_fill_batch_host: frame " + std::to_string(sc.bad) + " ends past frames_bytes");
    const uint64_t lo = sc.lo, hi = sc.hi + extra;
    fs_status st = begin_host_call(ctx);
    if (st == FS_SUCCESS) st = ensure_pinned(ctx, n);
    if (st != FS_SUCCESS) return st;
    uint64_t* h_off = reinterpret_cast<uint64_t*>(ctx->h_pin);
    uint32_t* h_len = reinterpret_cast<uint32_t*>(ctx->h_pin + (size_t)n * 8);
    fs_digest* h_out = reinterpret_cast<fs_digest*>(ctx->h_pin + (size_t)n * 12);
    uint8_t* h_st = ctx->h_pin + (size_t)n * 20;
    std::memcpy(h_off, offsets, (size_t)n * 8);
    std::memcpy(h_len, lengths, (size_t)n * 4);
    Staged s;
    st = stage_batch(ctx, frames, frames_bytes, lo, hi, h_off, h_len, n, s);
    if (st != FS_SUCCESS) return st;
    FS_HIP_DRAIN(ctx, launch(ctx, s.base, s.d_off, s.d_len, n, mtu, s.d_out, status ? s.d_st : nullptr, s.ks,
                             framesum::FsOp::kFill, s.base, flags));
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(frames + lo, s.base + lo, hi - lo, hipMemcpyDeviceToHost, s.ks));
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(h_out, s.d_out, (size_t)n * sizeof(fs_digest), hipMemcpyDeviceToHost, s.ks));
    if (status) FS_HIP_DRAIN(ctx, hipMemcpyAsync(h_st, s.d_st, n, hipMemcpyDeviceToHost, s.ks));
    st = finish_staged(ctx, s);
    if (st != FS_SUCCESS) return st;
    std::memcpy(out, h_out, (size_t)n * sizeof(fs_digest));
    if (status) std::memcpy(status, h_st, n);
    return FS_SUCCESS;
}

fs_status fs_digest_batch_multi(fs_ctx* const* ctxs, int nctx, const uint8_t* frames, uint64_t frames_bytes,
                                const uint64_t* offsets, const uint32_t* lengths, uint32_t n, uint32_t mtu,
                                fs_digest* out, uint8_t* status) {
    if (!ctxs || nctx <= 0) return FS_E_INVALID;
    for (int k = 0; k < nctx; ++k) {
        if (!ctxs[k]) return FS_E_INVALID;
        ctxs[k]->err.clear();
        for (int j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k])
                return set_err(ctxs[k], FS_E_INVALID, "fs_digest_batch_multi: a context appears twice in ctxs");
    }
    if (n == 0) return FS_SUCCESS;
    if (n > kMaxFrames)
        return set_err(ctxs[0], FS_E_INVALID, "fs_digest_batch_multi: n too large (at most 2^31 frames per call)");
    if (!frames || !offsets || !lengths || !out)
        return set_err(ctxs[0], FS_E_INVALID, "fs_digest_batch_multi: null pointer");
    const uint32_t bad = framesum::plan::first_frame_out_of_range(offsets, lengths, n, frames_bytes);
    if (bad < n)
        return set_err(ctxs[0], FS_E_INVALID, "fs_digest_batch_multi: frame " + std::to_string(bad) + " ends past frames_bytes");
    // block k = a run of frames in buffer order holding about 1/nctx of the bytes (one H2D
    // stream per GPU over its own bytes); unordered batches are ordered by offset first and
    // their results scattered back to batch order
    framesum::plan::MultiPlan plan;
    struct Block {
        std::vector<uint64_t> off;
        std::vector<uint32_t> len;
        std::vector<fs_digest> dig;
        std::vector<uint8_t> st;
    };
    std::vector<Block> blk;
    std::vector<fs_status> st;
    try {
        framesum::plan::multi_blocks(offsets, lengths, n, nctx, plan);
        blk.resize(nctx);
        st.assign(nctx, FS_SUCCESS);
        if (!plan.order.empty()) {
            for (int k = 0; k < nctx; ++k) {
                Block& b = blk[k];
                const uint32_t p0 = plan.cut[k], p1 = plan.cut[k + 1];
                b.off.resize(p1 - p0);
                b.len.resize(p1 - p0);
                b.dig.resize(p1 - p0);
                b.st.resize(status ? p1 - p0 : 0);
                for (uint32_t p = p0; p < p1; ++p) {
                    b.off[p - p0] = offsets[plan.order[p]];
                    b.len[p - p0] = lengths[plan.order[p]];
                }
            }
        }
    } catch (const std::bad_alloc&) {
        return set_err(ctxs[0], FS_E_NOMEM, "fs_digest_batch_multi: out of host memory");
    }
    auto run_block = [&](int k) {
        const uint32_t p0 = plan.cut[k], p1 = plan.cut[k + 1];
        if (p1 <= p0) return;
        if (plan.order.empty()) {
            st[k] = fs_digest_batch_host(ctxs[k], frames, frames_bytes, offsets + p0, lengths + p0, p1 - p0, mtu,
                                         out + p0, status ? status + p0 : nullptr);
            return;
        }
        Block& b = blk[k];
        st[k] = fs_digest_batch_host(ctxs[k], frames, frames_bytes, b.off.data(), b.len.data(), p1 - p0, mtu,
                                     b.dig.data(), status ? b.st.data() : nullptr);
        if (st[k] != FS_SUCCESS) return;
        for (uint32_t p = p0; p < p1; ++p) {
            out[plan.order[p]] = b.dig[p - p0];
            if (status) status[plan.order[p]] = b.st[p - p0];
        }
    };
    // One host thread per block beyond the first; if a thread cannot be started, its block runs
    // on the calling thread instead (never an exception across the ABI, no joinable thread left).
    std::vector<std::thread> workers;
    std::vector<int> inline_blocks;
    try {
        workers.reserve(nctx - 1);
        inline_blocks.reserve(nctx);
    } catch (const std::bad_alloc&) {
        return set_err(ctxs[0], FS_E_NOMEM, "fs_digest_batch_multi: out of host memory");
    }
    for (int k = 1; k < nctx; ++k) {
        try {
            workers.emplace_back(run_block, k);
        } catch (const std::system_error&) {
            inline_blocks.push_back(k);
        }
    }
    run_block(0);
    for (int k : inline_blocks) run_block(k);
    for (auto& w : workers) w.join();
    for (int k = 0; k < nctx; ++k)
        if (st[k] != FS_SUCCESS) return st[k];
    return FS_SUCCESS;
}

fs_status fs_deinterleave(fs_ctx* ctx, const uint8_t* gathered, uint32_t nshards, uint64_t n, fs_digest* out,
                          uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (n == 0) return FS_SUCCESS;
    if (!gathered || !out || nshards == 0) return set_err(ctx, FS_E_INVALID, "fs_deinterleave: null pointer or no shards");
    FS_HIP(ctx, hipSetDevice(ctx->device));
    FS_HIP(ctx, framesum::launch_deinterleave(gathered, nshards, n, out, status, reinterpret_cast<hipStream_t>(stream)));
    return FS_SUCCESS;
}

fs_status fs_ctx_set_workgroups(fs_ctx* ctx, int workgroups) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (workgroups < 0) return set_err(ctx, FS_E_INVALID, "fs_ctx_set_workgroups: workgroups must be >= 0");
    ctx->workgroups = workgroups;
    return FS_SUCCESS;
}

fs_status fs_ctx_set_kernel(fs_ctx* ctx, int variant) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (variant != 0 && variant != 2 && variant != 3 && variant != 4 && variant != 8)
        return set_err(ctx, FS_E_INVALID, "fs_ctx_set_kernel: variant must be 0 (automatic), 2, 3, 4 or 8");
    ctx->force_kernel = variant;
    return FS_SUCCESS;
}

int fs_ctx_last_kernel(const fs_ctx* ctx) {
    if (!ctx || !ctx->h_report) return FS_E_INVALID;
    return (int)ctx->choice.chosen;
}

#ifdef FS_TEST_HOOKS
// Test library only (-DFS_TEST_HOOKS): fs_digest_batch_host on ctx fails at chunk `chunk` (-1: never).
fs_status fs_test_set_fault(fs_ctx* ctx, long chunk) {
    if (!ctx) return FS_E_INVALID;
    ctx->fault_chunk = chunk;
    return FS_SUCCESS;
}
// ... and the context's kernel choice set to any choose() force value (framesum_choice.h), e.g. kForceSmallExact (16):
// the small-frame kernel for every launch, whatever the reports say (the parity suite's
// "small_exact" column runs every case through that kernel's own long-frame path).
fs_status fs_test_set_kernel_exact(fs_ctx* ctx, int force) {
    if (!ctx) return FS_E_INVALID;
    ctx->force_kernel = force;
    return FS_SUCCESS;
}
// ... and which path the latest fs_digest_batch_host took: 1 staged in one chunk, 2 read in place,
// 3 chunked (0 before the first call).
int fs_test_last_host_path(const fs_ctx* ctx) { return ctx ? ctx->last_host_path : -1; }
// ... the flow table's hash ANDed with `mask` before it becomes a slot index (0: every key starts at
// slot 0, so every insert probes linearly; the results of fs_coalesce_flows_batch do not change).
fs_status fs_test_set_flow_hash_mask(fs_ctx* ctx, uint32_t mask) {
    if (!ctx) return FS_E_INVALID;
    ctx->flow_hash_mask = mask;
    return FS_SUCCESS;
}
// ... and which groups of fs_coalesce_flows_batch's launches a call enqueues (kFlowStep* bits,
// framesum_internal.h; anything but all of them also leaves the digest launch out): 2 repeats the
// sort alone on the keys the call before left in the context's scratch, for tools/coalesce_bench.py.
fs_status fs_test_set_flow_steps(fs_ctx* ctx, uint32_t steps) {
    if (!ctx || steps == 0 || (steps & ~framesum::kFlowStepsAll)) return FS_E_INVALID;
    ctx->flow_steps = steps;
    return FS_SUCCESS;
}
#endif

fs_status fs_host_alloc(fs_ctx* ctx, uint64_t bytes, void** out) {
    if (!ctx || !out) return FS_E_INVALID;
    *out = nullptr;
    // Mapped (the in-place read and the direct result writes take its device address) and portable
    // (fs_digest_batch_multi's other contexts address it too). Coarse-grained: a kernel may cache its
    // lines in L2, but every launch begins with a system-scope acquire (HIP's dispatch packets), which
    // invalidates them, so a buffer the caller refills between calls is read anew
    // (test_host_inplace_refilled_buffer runs 200 refills of one buffer through the in-place path).
    if (hipHostMalloc(out, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess)
        return set_err(ctx, FS_E_NOMEM, "hipHostMalloc failed");
    return FS_SUCCESS;
}

fs_status fs_host_free(fs_ctx* ctx, void* p) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (p) FS_HIP(ctx, hipHostFree(p));
    return FS_SUCCESS;
}

}  // extern "C"
