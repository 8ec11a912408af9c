// framesum C ABI (include/framesum_send.h) -- the ring send: fs_send_rings_layout, fs_send_rings_batch
// and fs_send_rings_batch_host (kernel: framesum_send.hip; checks, the per-socket rule and the layout:
// framesum_send.h). The calls stage through the TX frame build's blocks and device buffers
// (framesum_api_tx.cpp).
#include <functional>
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

// Stage a checked batch with frames to build and enqueue its copy and its one kernel.
static fs_status send_enqueue(fs_ctx* ctx, const fs_tx_sock* socks, uint32_t n_socks, const framesum::send::Layout& L,
                              uint32_t mtu, uint32_t flags, uint32_t align, const TxDevice& t) {
    namespace snd = framesum::send;
    const framesum::segment::Block b = snd::block_of(L.n_recs, L.id_entries);
    const auto fill = [&](uint8_t* h_block) { snd::stage(socks, n_socks, flags, align, b, h_block); };
    const auto launch = [&](const uint8_t* d_block, int workgroups) {
        return framesum::launch_send_rings(d_block, b, L.n_recs, (uint32_t)L.n_frames, t.src, t.frames, t.offsets, t.lengths,
                                           t.out, t.status, mtu, flags, align, ctx->d_seg_tables, workgroups, t.stream);
    };
    return tx_enqueue(ctx, b.bytes, std::ref(fill), std::ref(launch), "fs_send_rings_batch: launch", t.stream);
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
    return send_enqueue(ctx, socks, n_socks, L, mtu, flags, align,
                        TxDevice{rings, frames, offsets, lengths, out, status, reinterpret_cast<hipStream_t>(stream)});
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
    const auto enqueue = [&](const TxDevice& t) { return send_enqueue(ctx, socks, n_socks, L, mtu, flags, align, t); };
    // (the ring bytes the frames carry are L's read span)
    return tx_host_call(ctx, rings, L.read_lo, L.read_hi, L.n_frames, L.frames_bytes, L.written != L.frames_bytes, frames,
                        offsets, lengths, out, status, std::ref(enqueue));
}
