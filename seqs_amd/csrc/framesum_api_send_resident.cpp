// framesum C ABI (include/framesum_send_resident.h) -- the ring send from device-resident sockets:
// fs_send_rings_resident (kernels: framesum_send_resident.hip; their arithmetic and the scratch layout:
// framesum_send_resident.h). The host checks the call's own arguments only: everything that depends on a
// socket is decided on the device.
#include <string>

#include "framesum_ctx.h"
#include "framesum_send_resident.h"

using namespace framesum::host;

fs_status fs_send_rings_resident(fs_ctx* ctx, fs_tx_sock* socks, uint32_t n_socks, const fs_rx_sock_out* rx_socks_out,
                                 const fs_rx_snd_out* rx_snd_out, const uint32_t* rx_index, uint32_t n_rx,
                                 const uint8_t* rings, uint64_t rings_bytes, uint32_t mtu, uint32_t flags, uint32_t align,
                                 uint8_t* frames, uint64_t frames_bytes, uint32_t frames_cap, uint64_t* offsets,
                                 uint32_t* lengths, fs_digest* out, uint8_t* status, fs_tx_sock_out* socks_out,
                                 fs_tx_totals* totals, void* stream) {
    namespace res = framesum::resident;
    const std::string fn = "fs_send_rings_resident: ";
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    if (flags & ~res::kCallFlags) return set_err(ctx, FS_E_INVALID, fn + "flags must be FS_FCS_APPEND, FS_TX_WRITEBACK or both");
    if (!framesum::segment::valid_align(align)) return set_err(ctx, FS_E_INVALID, fn + "align must be a power of two from 1 to 4096");
    if (n_socks > FS_SEND_MAX_SOCKS) return set_err(ctx, FS_E_INVALID, fn + "n_socks above FS_SEND_MAX_SOCKS");
    if (frames_cap > res::kMaxFramesCap) return set_err(ctx, FS_E_INVALID, fn + "frames_cap above 2^31");
    if (n_socks > 0 && (!socks || !socks_out || !totals)) return set_err(ctx, FS_E_INVALID, fn + "null socks, socks_out or totals");
    if (!rings && rings_bytes > 0) return set_err(ctx, FS_E_INVALID, fn + "null rings");
    if (!frames && frames_bytes > 0) return set_err(ctx, FS_E_INVALID, fn + "null frames");
    if (rx_snd_out && !rx_socks_out) return set_err(ctx, FS_E_INVALID, fn + "rx_snd_out without rx_socks_out");
    if (rx_index && !rx_socks_out) return set_err(ctx, FS_E_INVALID, fn + "rx_index without rx_socks_out");
    if (rx_socks_out && !rx_index && n_rx != n_socks)
        return set_err(ctx, FS_E_INVALID, fn + "n_rx must equal n_socks without rx_index");
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    FS_HIP(ctx, hipSetDevice(ctx->device));
    if (n_socks == 0) {
        if (totals) FS_HIP(ctx, hipMemsetAsync(totals, 0, sizeof(fs_tx_totals), s));
        return FS_SUCCESS;
    }
    fs_status st = seg_tables(ctx);
    if (st != FS_SUCCESS) return st;
    const res::Scratch sl = res::scratch_of(n_socks, frames_cap);
    st = ctx->sr_scratch.grow(ctx, sl.bytes, "hipMalloc of the resident send's scratch");
    if (st != FS_SUCCESS) return st;
    res::Call c{};
    c.socks = socks;
    c.rx_socks_out = rx_socks_out;
    c.rx_snd_out = rx_snd_out;
    c.rx_index = rx_index;
    c.socks_out = socks_out;
    c.totals = totals;
    c.rings_bytes = rings_bytes;
    c.frames_bytes = frames_bytes;
    c.n_socks = n_socks;
    c.n_rx = n_rx;
    c.frames_cap = frames_cap;
    c.flags = flags;
    c.align = align;
    // the grids' caps: the plan kernels' as the RX calls' launches (8 workgroups of 256 lanes per CU), the
    // frame kernel's as the TX frame build's (two per CU), both unless fs_ctx_set_workgroups asks for fewer
    const int plan_wgs = ctx->workgroups > 0 ? ctx->workgroups : 8 * ctx->num_cus;
    const int tx_wgs = ctx->workgroups > 0 && ctx->workgroups < 2 * ctx->num_cus ? ctx->workgroups : 2 * ctx->num_cus;
    const hipError_t e = framesum::launch_send_resident(c, ctx->sr_scratch.p, sl, rings, frames, offsets, lengths, out, status,
                                                        mtu, ctx->d_seg_tables, plan_wgs, tx_wgs, s);
    if (e != hipSuccess) return hip_err(ctx, e, "fs_send_rings_resident: launch");
    return FS_SUCCESS;
}
