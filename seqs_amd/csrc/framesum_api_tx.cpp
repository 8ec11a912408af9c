// framesum C ABI (include/framesum.h) -- the TX frame build: fs_segment_layout, fs_segment_batch and
// fs_segment_batch_host (kernel: framesum_segment.hip; checks and layout: framesum_segment.h), and
// what they share with the ring send (framesum_api_send.cpp): the staging blocks, the tables, the
// enqueue of a staged batch and the host form's device round trip.
#include <functional>
#include <new>
#include <string>

#include "framesum_ctx.h"
#include "framesum_segment.h"

using namespace framesum::host;

// Every check of a segment call that needs no device: flags, align, each send, the totals.
static fs_status segment_check(fs_ctx* ctx, const char* fn, const fs_tx_send* sends, uint32_t n_sends, uint32_t flags,
                               uint32_t align, bool have_payload, uint64_t payload_bytes, framesum::segment::Layout& L) {
    namespace seg = framesum::segment;
    if (!seg::valid_flags(flags)) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": flags must be 0 or FS_FCS_APPEND");
    if (!seg::valid_align(align))
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": align must be a power of two from 1 to 4096");
    if (!sends) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null pointer");
    L = seg::layout(sends, n_sends, flags, align, have_payload, payload_bytes);
    if (L.bad != seg::kGood)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": send " + std::to_string(L.bad_send) + ": " + seg::bad_text(L.bad));
    return FS_SUCCESS;
}

// A staging block of at least `bytes` bytes whose previous kernel has ended.
fs_status framesum::host::stage_block(fs_ctx* ctx, uint64_t bytes, SegStage** out) {
    SegStage* pick = nullptr;
    for (SegStage& sg : ctx->seg_stage) {
        if (sg.used) {
            const hipError_t q = hipEventQuery(sg.done);
            if (q == hipErrorNotReady) continue;
            if (q != hipSuccess) return hip_err(ctx, q, "hipEventQuery of a staging block");
            sg.used = false;
        }
        if (!pick || (pick->cap < bytes && sg.cap >= bytes)) pick = &sg;
        if (pick->cap >= bytes) break;
    }
    if (!pick) {  // every block is in flight: wait for the oldest
        pick = &ctx->seg_stage[ctx->seg_next];
        ctx->seg_next = (ctx->seg_next + 1) % kSegStages;
        FS_HIP(ctx, hipEventSynchronize(pick->done));
        pick->used = false;
    }
    if (!pick->done) FS_HIP(ctx, hipEventCreateWithFlags(&pick->done, hipEventDisableTiming));
    if (pick->cap < bytes) {
        if (pick->h) (void)hipHostFree(pick->h);
        (void)hipFree(pick->d);
        pick->h = nullptr;
        pick->d = nullptr;
        pick->cap = 0;
        const uint64_t cap = (bytes + 4095) & ~4095ull;
        if (hipHostMalloc(reinterpret_cast<void**>(&pick->h), cap, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(&pick->d, cap) != hipSuccess)
            return set_err(ctx, FS_E_NOMEM, "staging block allocation failed");
        pick->cap = cap;
    }
    *out = pick;
    return FS_SUCCESS;
}

// The frame-building kernels' table basis on the device, built on the context's first such call.
fs_status framesum::host::seg_tables(fs_ctx* ctx) {
    if (ctx->d_seg_tables) return FS_SUCCESS;
    framesum::SegTables* h = new (std::nothrow) framesum::SegTables;
    if (!h) return set_err(ctx, FS_E_NOMEM, "frame build: out of host memory");
    framesum::build_segment_tables(h);
    hipError_t e = hipMalloc(&ctx->d_seg_tables, sizeof(framesum::SegTables));
    if (e == hipSuccess) e = hipMemcpy(ctx->d_seg_tables, h, sizeof(framesum::SegTables), hipMemcpyHostToDevice);
    delete h;
    if (e != hipSuccess) {
        (void)hipFree(ctx->d_seg_tables);
        ctx->d_seg_tables = nullptr;
        return hip_err(ctx, e, "frame build: table upload");
    }
    return FS_SUCCESS;
}

fs_status framesum::host::tx_enqueue(fs_ctx* ctx, uint64_t block_bytes, const std::function<void(uint8_t*)>& fill,
                                     const std::function<hipError_t(const uint8_t*, int)>& launch, const char* launch_what,
                                     hipStream_t stream) {
    const fs_status tst = seg_tables(ctx);
    if (tst != FS_SUCCESS) return tst;
    // two workgroups per CU (their tables fit its LDS twice) unless fs_ctx_set_workgroups caps the grid
    const int wgs = ctx->workgroups > 0 && ctx->workgroups < 2 * ctx->num_cus ? ctx->workgroups : 2 * ctx->num_cus;
    return staged_launch(ctx, block_bytes, stream, launch_what, fill, [&](const uint8_t* d_block) { return launch(d_block, wgs); });
}

fs_status framesum::host::tx_host_call(fs_ctx* ctx, const uint8_t* src, uint64_t lo, uint64_t hi, uint64_t n,
                                       uint64_t frames_bytes, bool gaps, uint8_t* frames, uint64_t* offsets, uint32_t* lengths,
                                       fs_digest* out, uint8_t* status,
                                       const std::function<fs_status(const TxDevice&)>& enqueue) {
    fs_status st = begin_host_call(ctx);
    if (st == FS_SUCCESS) st = ctx->seg_payload.grow(ctx, hi - lo);
    if (st == FS_SUCCESS) st = ctx->seg_frames.grow(ctx, frames_bytes);
    if (st == FS_SUCCESS) st = ctx->seg_arrays.grow(ctx, n * 21);
    if (st != FS_SUCCESS) return st;
    ctx->host_dirty = true;  // until this call has waited for all of its work
    const hipStream_t ks = ctx->compute_stream;
    // pinned memory (fs_host_alloc) is copied from and to directly; pageable memory goes through the
    // runtime's own pinned staging
    if (hi > lo) FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->seg_payload.p, src + lo, hi - lo, hipMemcpyHostToDevice, ks));
    // the kernel writes frame and FCS bytes only: when the slots leave gaps (align > 1), the span
    // goes in first so that the copy back returns the caller's own bytes there
    if (gaps) FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->seg_frames.p, frames, frames_bytes, hipMemcpyHostToDevice, ks));
    uint64_t* d_off = ctx->seg_arrays.as<uint64_t>();
    fs_digest* d_out = ctx->seg_arrays.as<fs_digest>(n * 8);
    uint32_t* d_len = ctx->seg_arrays.as<uint32_t>(n * 16);
    uint8_t* d_st = ctx->seg_arrays.p + n * 20;
    const uint8_t* base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(ctx->seg_payload.p) - lo);
    st = enqueue(TxDevice{base, ctx->seg_frames.p, offsets ? d_off : nullptr, lengths ? d_len : nullptr,
                          out ? d_out : nullptr, status ? d_st : nullptr, ks});
    if (st != FS_SUCCESS) {
        drain_host_streams(ctx);
        return st;
    }
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(frames, ctx->seg_frames.p, frames_bytes, hipMemcpyDeviceToHost, ks));
    if (offsets) FS_HIP_DRAIN(ctx, hipMemcpyAsync(offsets, d_off, n * 8, hipMemcpyDeviceToHost, ks));
    if (lengths) FS_HIP_DRAIN(ctx, hipMemcpyAsync(lengths, d_len, n * 4, hipMemcpyDeviceToHost, ks));
    if (out) FS_HIP_DRAIN(ctx, hipMemcpyAsync(out, d_out, n * sizeof(fs_digest), hipMemcpyDeviceToHost, ks));
    if (status) FS_HIP_DRAIN(ctx, hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, ks));
    FS_HIP_DRAIN(ctx, hipStreamSynchronize(ks));
    ctx->host_dirty = false;
    return FS_SUCCESS;
}

// Stage a checked batch and enqueue its copy and its one kernel.
static fs_status segment_enqueue(fs_ctx* ctx, const fs_tx_send* sends, uint32_t n_sends,
                                 const framesum::segment::Layout& L, uint32_t mtu, uint32_t flags, uint32_t align,
                                 const TxDevice& t) {
    namespace seg = framesum::segment;
    const seg::Block b = seg::block_of(n_sends, L.id_entries);
    const auto fill = [&](uint8_t* h_block) { seg::stage(sends, n_sends, flags, align, b, h_block); };
    const auto launch = [&](const uint8_t* d_block, int workgroups) {
        return framesum::launch_segment(d_block, b, n_sends, (uint32_t)L.n_frames, t.src, t.frames, t.offsets, t.lengths, t.out,
                                        t.status, mtu, flags, align, ctx->d_seg_tables, workgroups, t.stream);
    };
    return tx_enqueue(ctx, b.bytes, std::ref(fill), std::ref(launch), "fs_segment_batch: launch", t.stream);
}

fs_status fs_segment_layout(const fs_tx_send* sends, uint32_t n_sends, uint32_t flags, uint32_t align, uint64_t* n_frames,
                            uint64_t* frames_bytes) {
    g_create_err.clear();
    framesum::segment::Layout L;
    if (n_sends == 0) {
        if (!framesum::segment::valid_flags(flags) || !framesum::segment::valid_align(align))
            return set_err(nullptr, FS_E_INVALID, "fs_segment_layout: bad flags or align");
    } else {
        const fs_status st = segment_check(nullptr, "fs_segment_layout", sends, n_sends, flags, align, false, 0, L);
        if (st != FS_SUCCESS) return st;
    }
    if (n_frames) *n_frames = L.n_frames;
    if (frames_bytes) *frames_bytes = L.frames_bytes;
    return FS_SUCCESS;
}

// The checks fs_segment_batch and fs_segment_batch_host share, all before any device call.
static fs_status segment_args(fs_ctx* ctx, const char* fn, const fs_tx_send* sends, uint32_t n_sends, const uint8_t* payload,
                              uint64_t payload_bytes, uint32_t flags, uint32_t align, const uint8_t* frames,
                              uint64_t frames_bytes, framesum::segment::Layout& L) {
    const fs_status st = segment_check(ctx, fn, sends, n_sends, flags, align, true, payload_bytes, L);
    if (st != FS_SUCCESS) return st;
    if (!frames) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null pointer");
    if (!payload && L.payload > 0)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null payload");
    if (frames_bytes < L.frames_bytes)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": frames_bytes " + std::to_string(frames_bytes) +
                                              " is below the layout's " + std::to_string(L.frames_bytes));
    return FS_SUCCESS;
}

fs_status fs_segment_batch(fs_ctx* ctx, const fs_tx_send* sends, uint32_t n_sends, const uint8_t* payload,
                           uint64_t payload_bytes, uint32_t mtu, uint32_t flags, uint32_t align, uint8_t* frames,
                           uint64_t frames_bytes, uint64_t* offsets, uint32_t* lengths, fs_digest* out, uint8_t* status,
                           void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (n_sends == 0) return FS_SUCCESS;
    framesum::segment::Layout L;
    const fs_status st = segment_args(ctx, "fs_segment_batch", sends, n_sends, payload, payload_bytes, flags, align, frames,
                                      frames_bytes, L);
    if (st != FS_SUCCESS) return st;
    FS_HIP(ctx, hipSetDevice(ctx->device));
    return segment_enqueue(ctx, sends, n_sends, L, mtu, flags, align,
                           TxDevice{payload, frames, offsets, lengths, out, status, reinterpret_cast<hipStream_t>(stream)});
}

fs_status fs_segment_batch_host(fs_ctx* ctx, const fs_tx_send* sends, uint32_t n_sends, const uint8_t* payload,
                                uint64_t payload_bytes, uint32_t mtu, uint32_t flags, uint32_t align, uint8_t* frames,
                                uint64_t frames_bytes, uint64_t* offsets, uint32_t* lengths, fs_digest* out,
                                uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (n_sends == 0) return FS_SUCCESS;
    framesum::segment::Layout L;
    const fs_status ast = segment_args(ctx, "fs_segment_batch_host", sends, n_sends, payload, payload_bytes, flags, align,
                                       frames, frames_bytes, L);
    if (ast != FS_SUCCESS) return ast;
    // the payload bytes the sends use
    uint64_t lo = UINT64_MAX, hi = 0;
    for (uint32_t i = 0; i < n_sends; ++i) {
        if (sends[i].payload_len == 0) continue;
        const uint64_t o = sends[i].payload_off, e = o + sends[i].payload_len;
        lo = o < lo ? o : lo;
        hi = e > hi ? e : hi;
    }
    if (hi <= lo) lo = hi = 0;
    const auto enqueue = [&](const TxDevice& t) { return segment_enqueue(ctx, sends, n_sends, L, mtu, flags, align, t); };
    return tx_host_call(ctx, payload, lo, hi, L.n_frames, L.frames_bytes, L.written != L.frames_bytes, frames, offsets,
                        lengths, out, status, std::ref(enqueue));
}
