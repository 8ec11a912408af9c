// framesum C ABI (include/framesum_send.h) -- the ring send: fs_send_rings_layout, fs_send_rings_batch
// and fs_send_rings_batch_host (kernel: framesum_send.hip; checks, the per-socket rule and the layout:
// framesum_send.h). The calls stage through the TX frame build's blocks and device buffers
// (framesum_api_tx.cpp).
#include <string>

#include "framesum_ctx.h"
#include "framesum_send.h"

using namespace framesum::host;

// Every check of a ring send that needs no device, and with them socks_out (nullable).
static fs_status send_check(fs_ctx* ctx, const char* fn, const fs_tx_sock* socks, uint32_t n_socks, uint32_t flags,
                            uint32_t align, bool have_rings, uint64_t rings_bytes, fs_tx_sock_out* socks_out,
                            framesum::send::Layout& L) {
    namespace seg = framesum::segment;
    namespace snd = framesum::send;
    if (!seg::valid_flags(flags)) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": flags must be 0 or FS_FCS_APPEND");
    if (!seg::valid_align(align))
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": align must be a power of two from 1 to 4096");
    if (n_socks > FS_SEND_MAX_SOCKS) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": n_socks above FS_SEND_MAX_SOCKS");
    if (!socks) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null pointer");
    L = snd::layout(socks, n_socks, flags, align, have_rings, rings_bytes, socks_out);
    if (L.bad != snd::kGood)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": socket " + std::to_string(L.bad_sock) + ": " + snd::bad_text(L.bad));
    return FS_SUCCESS;
}

fs_status fs_send_rings_layout(const fs_tx_sock* socks, uint32_t n_socks, uint32_t flags, uint32_t align, uint64_t* n_frames,
                               uint64_t* frames_bytes, fs_tx_sock_out* socks_out) {
    g_create_err.clear();
    framesum::send::Layout L;
    if (n_socks == 0) {
        if (!framesum::segment::valid_flags(flags) || !framesum::segment::valid_align(align))
            return set_err(nullptr, FS_E_INVALID, "fs_send_rings_layout: bad flags or align");
    } else {
        const fs_status st = send_check(nullptr, "fs_send_rings_layout", socks, n_socks, flags, align, false, 0, socks_out, L);
        if (st != FS_SUCCESS) return st;
    }
    if (n_frames) *n_frames = L.n_frames;
    if (frames_bytes) *frames_bytes = L.frames_bytes;
    return FS_SUCCESS;
}

// The checks fs_send_rings_batch and fs_send_rings_batch_host share, all before any device call.
static fs_status send_args(fs_ctx* ctx, const char* fn, const fs_tx_sock* socks, uint32_t n_socks, const uint8_t* rings,
                           uint64_t rings_bytes, uint32_t flags, uint32_t align, const uint8_t* frames, uint64_t frames_bytes,
                           fs_tx_sock_out* socks_out, framesum::send::Layout& L) {
    const fs_status st = send_check(ctx, fn, socks, n_socks, flags, align, true, rings_bytes, socks_out, L);
    if (st != FS_SUCCESS) return st;
    if (L.n_frames == 0) return FS_SUCCESS;  // nothing to build
    if (!frames) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null pointer");
    if (!rings && L.data > 0) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null rings");
    if (frames_bytes < L.frames_bytes)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": frames_bytes " + std::to_string(frames_bytes) +
                                              " is below the layout's " + std::to_string(L.frames_bytes));
    return FS_SUCCESS;
}

// Stage a checked batch with frames to build and enqueue its copy and its one kernel on `stream`.
static fs_status send_enqueue(fs_ctx* ctx, const fs_tx_sock* socks, uint32_t n_socks, const framesum::send::Layout& L,
                              const uint8_t* rings, uint32_t mtu, uint32_t flags, uint32_t align, uint8_t* frames,
                              uint64_t* offsets, uint32_t* lengths, fs_digest* out, uint8_t* status, hipStream_t stream) {
    namespace snd = framesum::send;
    const fs_status tst = seg_tables(ctx);
    if (tst != FS_SUCCESS) return tst;
    const framesum::segment::Block b = snd::block_of(L.n_recs, L.id_entries);
    SegStage* sg = nullptr;
    const fs_status st = stage_block(ctx, b.bytes, &sg);
    if (st != FS_SUCCESS) return st;
    snd::stage(socks, n_socks, flags, align, b, sg->h);
    FS_HIP(ctx, hipMemcpyAsync(sg->d, sg->h, b.bytes, hipMemcpyHostToDevice, stream));
    // two workgroups per CU (their tables fit its LDS twice) unless fs_ctx_set_workgroups caps the grid
    const int wgs = ctx->workgroups > 0 && ctx->workgroups < 2 * ctx->num_cus ? ctx->workgroups : 2 * ctx->num_cus;
    sg->used = true;  // (from here on the block may be read by queued work)
    const hipError_t le = framesum::launch_send_rings(sg->d, b, L.n_recs, (uint32_t)L.n_frames, rings, frames, offsets, lengths,
                                                      out, status, mtu, flags, align, ctx->d_seg_tables, wgs, stream);
    const hipError_t re = hipEventRecord(sg->done, stream);
    if (le != hipSuccess) return hip_err(ctx, le, "fs_send_rings_batch: launch");
    if (re != hipSuccess) return hip_err(ctx, re, "hipEventRecord(sg->done, stream)");
    return FS_SUCCESS;
}

fs_status fs_send_rings_batch(fs_ctx* ctx, const fs_tx_sock* socks, uint32_t n_socks, const uint8_t* rings,
                              uint64_t rings_bytes, uint32_t mtu, uint32_t flags, uint32_t align, uint8_t* frames,
                              uint64_t frames_bytes, uint64_t* offsets, uint32_t* lengths, fs_digest* out, uint8_t* status,
                              fs_tx_sock_out* socks_out, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (n_socks == 0) return FS_SUCCESS;
    framesum::send::Layout L;
    const fs_status st = send_args(ctx, "fs_send_rings_batch", socks, n_socks, rings, rings_bytes, flags, align, frames,
                                   frames_bytes, socks_out, L);
    if (st != FS_SUCCESS || L.n_frames == 0) return st;
    FS_HIP(ctx, hipSetDevice(ctx->device));
    return send_enqueue(ctx, socks, n_socks, L, rings, mtu, flags, align, frames, offsets, lengths, out, status,
                        reinterpret_cast<hipStream_t>(stream));
}

fs_status fs_send_rings_batch_host(fs_ctx* ctx, const fs_tx_sock* socks, uint32_t n_socks, const uint8_t* rings,
                                   uint64_t rings_bytes, uint32_t mtu, uint32_t flags, uint32_t align, uint8_t* frames,
                                   uint64_t frames_bytes, uint64_t* offsets, uint32_t* lengths, fs_digest* out,
                                   uint8_t* status, fs_tx_sock_out* socks_out) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (n_socks == 0) return FS_SUCCESS;
    framesum::send::Layout L;
    const fs_status ast = send_args(ctx, "fs_send_rings_batch_host", socks, n_socks, rings, rings_bytes, flags, align, frames,
                                    frames_bytes, socks_out, L);
    if (ast != FS_SUCCESS || L.n_frames == 0) return ast;
    const uint64_t lo = L.read_lo, hi = L.read_hi;  // the ring bytes the frames carry
    const uint64_t n = L.n_frames;
    FS_HIP(ctx, hipSetDevice(ctx->device));
    fs_status st = begin_host_call(ctx);
    if (st == FS_SUCCESS) st = ctx->seg_payload.grow(ctx, hi - lo);
    if (st == FS_SUCCESS) st = ctx->seg_frames.grow(ctx, L.frames_bytes);
    if (st == FS_SUCCESS) st = ctx->seg_arrays.grow(ctx, n * 21);
    if (st != FS_SUCCESS) return st;
    ctx->host_dirty = true;  // until this call has waited for all of its work
    const hipStream_t ks = ctx->compute_stream;
    if (hi > lo) FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->seg_payload.p, rings + lo, hi - lo, hipMemcpyHostToDevice, ks));
    // the kernel writes frame and FCS bytes only: when the slots leave gaps (align > 1), the span
    // goes in first so that the copy back returns the caller's own bytes there
    if (L.written != L.frames_bytes)
        FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->seg_frames.p, frames, L.frames_bytes, hipMemcpyHostToDevice, ks));
    uint64_t* d_off = ctx->seg_arrays.as<uint64_t>();
    fs_digest* d_out = ctx->seg_arrays.as<fs_digest>(n * 8);
    uint32_t* d_len = ctx->seg_arrays.as<uint32_t>(n * 16);
    uint8_t* d_st = ctx->seg_arrays.p + n * 20;
    const uint8_t* base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(ctx->seg_payload.p) - lo);
    st = send_enqueue(ctx, socks, n_socks, L, base, mtu, flags, align, ctx->seg_frames.p, offsets ? d_off : nullptr,
                      lengths ? d_len : nullptr, out ? d_out : nullptr, status ? d_st : nullptr, ks);
    if (st != FS_SUCCESS) {
        drain_host_streams(ctx);
        return st;
    }
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(frames, ctx->seg_frames.p, L.frames_bytes, hipMemcpyDeviceToHost, ks));
    if (offsets) FS_HIP_DRAIN(ctx, hipMemcpyAsync(offsets, d_off, n * 8, hipMemcpyDeviceToHost, ks));
    if (lengths) FS_HIP_DRAIN(ctx, hipMemcpyAsync(lengths, d_len, n * 4, hipMemcpyDeviceToHost, ks));
    if (out) FS_HIP_DRAIN(ctx, hipMemcpyAsync(out, d_out, n * sizeof(fs_digest), hipMemcpyDeviceToHost, ks));
    if (status) FS_HIP_DRAIN(ctx, hipMemcpyAsync(status, d_st, n * 1, hipMemcpyDeviceToHost, ks));
    FS_HIP_DRAIN(ctx, hipStreamSynchronize(ks));
    ctx->host_dirty = false;
    return FS_SUCCESS;
}
