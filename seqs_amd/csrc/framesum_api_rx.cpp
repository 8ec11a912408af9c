// framesum C ABI (include/framesum.h) -- the two RX coalesce families: fs_coalesce_batch and
// fs_coalesce_batch_host (kernels: framesum_coalesce.hip), fs_coalesce_flows_batch and
// fs_coalesce_flows_batch_host (framesum_flows.hip), and what their host forms share -- and
// (include/framesum_deliver.h) the delivery into socket rings behind the second family:
// fs_deliver_flows_batch and fs_deliver_flows_batch_host (framesum_deliver.hip), and
// (include/framesum_recv.h) the receive call behind the delivery: fs_recv_flows_batch and
// fs_recv_flows_batch_host (framesum_recv.hip).
#include <algorithm>
#include <array>
#include <cstring>
#include <string>
#include <vector>

#include "framesum_ctx.h"
#include "framesum_deliver.h"
#include "framesum_flows.h"
#include "framesum_recv.h"

using namespace framesum::host;

// ---- What the two host forms share ----

// One copy back to the caller (skipped when the caller passed no array, or nothing is to come back).
struct D2H {
    void* dst;
    const void* src;
    uint64_t bytes;
};

// A checked host-staged coalesce call `fn` of either family: the batch staged through slot 0, the
// family's launches (`enqueue`), then what they wrote copied back. The forms differ in the type of
// their totals, in what lies behind the runs in `arrays` (the device result arrays: the totals, a run
// per frame, then `rest_per_frame` bytes per frame of the family's own), in whether totals are
// `consistent`, and in the copies `rest` adds for its own arrays.
template <class Totals, class Enqueue, class Consistent, class Rest>
static fs_status rx_host(fs_ctx* ctx, const char* fn, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                         const uint32_t* lengths, uint32_t n, uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs,
                         Totals* totals, fs_digest* out, uint8_t* status, DevBuf& arrays, uint32_t rest_per_frame,
                         Enqueue enqueue, Consistent consistent, Rest rest) {
    if (n == 0) {
        std::memset(totals, 0, sizeof(Totals));
        return FS_SUCCESS;
    }
    const framesum::plan::Scan sc = framesum::plan::scan_batch(offsets, lengths, n, frames_bytes);
    if (sc.bad < n)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": frame " + std::to_string(sc.bad) + " ends past frames_bytes");
    // the device payload buffer: payload_cap, or the most payload the batch can hold when that is less
    const uint64_t d_cap = std::min(payload_cap, framesum::plan::total_length(lengths, n));
    fs_status st = begin_host_call(ctx);
    if (st == FS_SUCCESS) st = ctx->co_payload.grow(ctx, d_cap);
    if (st == FS_SUCCESS) st = arrays.grow(ctx, sizeof(Totals) + (uint64_t)n * (sizeof(fs_rx_run) + rest_per_frame));
    if (st != FS_SUCCESS) return st;
    Staged s;
    st = stage_batch(ctx, frames, frames_bytes, sc.lo, sc.hi, offsets, lengths, n, s);
    if (st != FS_SUCCESS) return st;
    Totals* d_totals = arrays.as<Totals>();
    fs_rx_run* d_runs = arrays.as<fs_rx_run>(sizeof(Totals));
    uint8_t* d_rest = arrays.p + sizeof(Totals) + (uint64_t)n * sizeof(fs_rx_run);
    const uint8_t* d_copied = nullptr;
    st = enqueue(s, d_cap, d_runs, d_rest, d_totals, &d_copied);
    if (st != FS_SUCCESS) {
        drain_host_streams(ctx);
        return st;
    }
    // the totals and how far the payload got written decide what else comes back
    Totals t;
    uint64_t copied = 0;
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(&t, d_totals, sizeof t, hipMemcpyDeviceToHost, s.ks));
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(&copied, d_copied, 8, hipMemcpyDeviceToHost, s.ks));
    FS_HIP_DRAIN(ctx, hipStreamSynchronize(s.ks));
    if (copied > d_cap || !consistent(t)) {
        drain_host_streams(ctx);
        return set_err(ctx, FS_E_HIP, std::string(fn) + ": inconsistent totals from the device");
    }
    const auto back = [&](const D2H& c) {
        return c.dst && c.bytes ? hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s.ks) : hipSuccess;
    };
    FS_HIP_DRAIN(ctx, back({payload, ctx->co_payload.p, copied}));
    FS_HIP_DRAIN(ctx, back({runs, d_runs, (uint64_t)t.n_runs * sizeof(fs_rx_run)}));
    for (const D2H& c : rest(t, d_rest)) FS_HIP_DRAIN(ctx, back(c));
    FS_HIP_DRAIN(ctx, back({out, s.d_out, (uint64_t)n * sizeof(fs_digest)}));
    FS_HIP_DRAIN(ctx, back({status, s.d_st, n}));
    st = finish_staged(ctx, s);
    if (st == FS_SUCCESS) *totals = t;
    return st;
}

// ---- RX coalesce (fs_coalesce_batch / fs_coalesce_batch_host) ----

// Every check of a coalesce call, none of which needs a device. An empty batch needs only `totals`.
static fs_status coalesce_check(fs_ctx* ctx, const char* fn, const void* frames, const void* offsets, const void* lengths,
                                uint32_t n, uint32_t flags, const void* payload, uint64_t payload_cap, const void* runs,
                                const void* totals, bool aligned) {
    if (flags & ~(uint32_t)FS_RX_FCS) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": flags must be 0 or FS_RX_FCS");
    if (n > kMaxFrames) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": n too large (at most 2^31 frames per call)");
    if (!totals) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null pointer");
    if (n == 0) return FS_SUCCESS;
    if (!frames || !offsets || !lengths || !runs) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null pointer");
    if (!payload && payload_cap != 0) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null payload with a non-zero payload_cap");
    if (aligned && (reinterpret_cast<uintptr_t>(frames) & 3u))
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": frames must be 4-byte aligned");
    return FS_SUCCESS;
}

// `out` and `status` of a device-resident call that passes none: the context's own.
static fs_status spare_results(fs_ctx* ctx, uint32_t n, fs_digest*& out, uint8_t*& status) {
    if (out && status) return FS_SUCCESS;
    const fs_status st = ctx->co_results.grow(ctx, (uint64_t)n * 9);
    if (st != FS_SUCCESS) return st;
    if (!out) out = ctx->co_results.as<fs_digest>();
    if (!status) status = ctx->co_results.p + (uint64_t)n * 8;
    return FS_SUCCESS;
}

// The digest launch and the coalesce launches of a checked, non-empty device-resident batch on `stream`.
// `d_copied` (nullable): where on the device the count of written payload bytes lies.
static fs_status coalesce_enqueue(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                  uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                                  fs_rx_run* runs, uint32_t* run_of, fs_rx_totals* totals, fs_digest* out, uint8_t* status,
                                  hipStream_t stream, const uint8_t** d_copied = nullptr) {
    const framesum::CoScratch s = framesum::coalesce_scratch(n);
    fs_status st = ctx->co_scratch.grow(ctx, s.bytes);
    if (st == FS_SUCCESS) st = spare_results(ctx, n, out, status);
    if (st != FS_SUCCESS) return st;
    if (d_copied) *d_copied = ctx->co_scratch.p + s.copied;
    FS_HIP(ctx, launch(ctx, frames, offsets, lengths, n, mtu, out, status, stream,
                       (flags & FS_RX_FCS) ? framesum::FsOp::kFcs : framesum::FsOp::kDigest, nullptr, 0));
    // up to 8 workgroups of 256 lanes per CU unless fs_ctx_set_workgroups caps the grids
    const int wgs = ctx->workgroups > 0 ? ctx->workgroups : 8 * ctx->num_cus;
    FS_HIP(ctx, framesum::launch_coalesce(frames, offsets, lengths, n, flags, status, payload, payload_cap, runs, run_of,
                                          totals, ctx->co_scratch.p, wgs, stream));
    return FS_SUCCESS;
}

fs_status fs_coalesce_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                            uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                            fs_rx_run* runs, uint32_t* run_of, fs_rx_totals* totals, fs_digest* out, uint8_t* status,
                            void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    const fs_status st = coalesce_check(ctx, "fs_coalesce_batch", frames, offsets, lengths, n, flags, payload, payload_cap,
                                        runs, totals, true);
    if (st != FS_SUCCESS) return st;
    FS_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        FS_HIP(ctx, hipMemsetAsync(totals, 0, sizeof(fs_rx_totals), reinterpret_cast<hipStream_t>(stream)));
        return FS_SUCCESS;
    }
    return coalesce_enqueue(ctx, frames, offsets, lengths, n, mtu, flags, payload, payload_cap, runs, run_of, totals, out,
                            status, reinterpret_cast<hipStream_t>(stream));
}

fs_status fs_coalesce_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                 const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload,
                                 uint64_t payload_cap, fs_rx_run* runs, uint32_t* run_of, fs_rx_totals* totals,
                                 fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    const char* const fn = "fs_coalesce_batch_host";
    const fs_status ast =
        coalesce_check(ctx, fn, frames, offsets, lengths, n, flags, payload, payload_cap, runs, totals, false);
    if (ast != FS_SUCCESS) return ast;
    // behind the runs: run_of (4 per frame)
    return rx_host(
        ctx, fn, frames, frames_bytes, offsets, lengths, n, payload, payload_cap, runs, totals, out, status, ctx->co_arrays, 4,
        [&](const Staged& s, uint64_t d_cap, fs_rx_run* d_runs, uint8_t* d_rest, fs_rx_totals* d_totals, const uint8_t** d_copied) {
            return coalesce_enqueue(ctx, s.base, s.d_off, s.d_len, n, mtu, flags, ctx->co_payload.p, d_cap, d_runs,
                                    run_of ? reinterpret_cast<uint32_t*>(d_rest) : nullptr, d_totals, s.d_out, s.d_st, s.ks,
                                    d_copied);
        },
        [&](const fs_rx_totals& t) { return t.n_runs <= n; },
        [&](const fs_rx_totals&, const uint8_t* d_rest) { return std::array<D2H, 1>{{{run_of, d_rest, (uint64_t)n * 4}}}; });
}

// ---- Flow-aware RX coalesce (fs_coalesce_flows_batch / fs_coalesce_flows_batch_host) ----

static fs_status flows_check(fs_ctx* ctx, const char* fn, const void* frames, const void* offsets, const void* lengths,
                             uint32_t n, uint32_t flags, const void* payload, uint64_t payload_cap, const void* runs,
                             const void* order, const void* totals, bool aligned) {
    if (n > framesum::flows::kMaxFrames)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": n too large (at most 2^30 frames per call)");
    const fs_status st =
        coalesce_check(ctx, fn, frames, offsets, lengths, n, flags, payload, payload_cap, runs, totals, aligned);
    if (st != FS_SUCCESS) return st;
    if (n != 0 && !order) return set_err(ctx, FS_E_INVALID, std::string(fn) + ": null pointer");  // (as `runs`)
    return FS_SUCCESS;
}

// The digest launch and the flow coalesce launches of a checked, non-empty device-resident batch on
// `stream`. `d_copied`: as coalesce_enqueue's. `layout` (nullable): where in the context's scratch the
// launches leave their per-slot arrays, for the delivery launches behind them.
static fs_status flows_enqueue(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                               uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                               fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                               fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, hipStream_t stream,
                               const uint8_t** d_copied = nullptr, framesum::FlowScratch* layout = nullptr) {
    const framesum::FlowScratch s = framesum::flows_scratch(n);
    if (layout) *layout = s;
    if (s.sort_bytes == 0) return set_err(ctx, FS_E_HIP, "fs_coalesce_flows_batch: the sort reports no temporary storage size");
    fs_status st = ctx->fl_scratch.grow(ctx, s.bytes);
    if (st == FS_SUCCESS) st = spare_results(ctx, n, out, status);
    if (st != FS_SUCCESS) return st;
    if (d_copied) *d_copied = ctx->fl_scratch.p + s.copied;
    if (ctx->flow_steps == framesum::kFlowStepsAll)
        FS_HIP(ctx, launch(ctx, frames, offsets, lengths, n, mtu, out, status, stream,
                           (flags & FS_RX_FCS) ? framesum::FsOp::kFcs : framesum::FsOp::kDigest, nullptr, 0));
    const int wgs = ctx->workgroups > 0 ? ctx->workgroups : 8 * ctx->num_cus;
    FS_HIP(ctx, framesum::launch_coalesce_flows(frames, offsets, lengths, n, flags, status, payload, payload_cap, runs, flows,
                                                order, run_of, totals, ctx->fl_scratch.p, s, ctx->flow_hash_mask, wgs,
                                                ctx->flow_steps, stream));
    return FS_SUCCESS;
}

fs_status fs_coalesce_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                  uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                                  fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                  fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    const fs_status st = flows_check(ctx, "fs_coalesce_flows_batch", frames, offsets, lengths, n, flags, payload,
                                     payload_cap, runs, order, totals, true);
    if (st != FS_SUCCESS) return st;
    FS_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        FS_HIP(ctx, hipMemsetAsync(totals, 0, sizeof(fs_rx_flow_totals), reinterpret_cast<hipStream_t>(stream)));
        return FS_SUCCESS;
    }
    return flows_enqueue(ctx, frames, offsets, lengths, n, mtu, flags, payload, payload_cap, runs, flows, order, run_of,
                         totals, out, status, reinterpret_cast<hipStream_t>(stream));
}

fs_status fs_coalesce_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes,
                                       const uint64_t* offsets, const uint32_t* lengths, uint32_t n, uint32_t mtu,
                                       uint32_t flags, uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs,
                                       fs_rx_flow* flows, uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals,
                                       fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    const char* const fn = "fs_coalesce_flows_batch_host";
    const fs_status ast =
        flows_check(ctx, fn, frames, offsets, lengths, n, flags, payload, payload_cap, runs, order, totals, false);
    if (ast != FS_SUCCESS) return ast;
    // behind the runs, per frame: a flow (32), order (4), run_of (4)
    const uint64_t at_order = (uint64_t)n * 32, at_run_of = (uint64_t)n * 36;
    return rx_host(
        ctx, fn, frames, frames_bytes, offsets, lengths, n, payload, payload_cap, runs, totals, out, status, ctx->fl_arrays, 40,
        [&](const Staged& s, uint64_t d_cap, fs_rx_run* d_runs, uint8_t* d_rest, fs_rx_flow_totals* d_totals,
            const uint8_t** d_copied) {
            return flows_enqueue(ctx, s.base, s.d_off, s.d_len, n, mtu, flags, ctx->co_payload.p, d_cap, d_runs,
                                 flows ? reinterpret_cast<fs_rx_flow*>(d_rest) : nullptr,
                                 reinterpret_cast<uint32_t*>(d_rest + at_order),
                                 run_of ? reinterpret_cast<uint32_t*>(d_rest + at_run_of) : nullptr, d_totals, s.d_out, s.d_st,
                                 s.ks, d_copied);
        },
        [&](const fs_rx_flow_totals& t) { return t.n_accepted <= n && t.n_runs <= t.n_accepted && t.n_flows <= t.n_runs; },
        [&](const fs_rx_flow_totals& t, const uint8_t* d_rest) {
            return std::array<D2H, 3>{{{flows, d_rest, (uint64_t)t.n_flows * sizeof(fs_rx_flow)},
                                       {order, d_rest + at_order, (uint64_t)t.n_accepted * 4},
                                       {run_of, d_rest + at_run_of, (uint64_t)n * 4}}};
        });
}

// ---- In-order TCP delivery (fs_deliver_flows_batch / fs_deliver_flows_batch_host, include/framesum_deliver.h) ----

namespace dl = framesum::deliver;

// Every check of a delivery call: the flow call's, then the socket list's (framesum_deliver.h), which
// also builds the socket table `table` and gives the span of `rings` the listed rings cover.
static fs_status deliver_check(fs_ctx* ctx, const char* fn, const void* frames, const void* offsets, const void* lengths,
                               uint32_t n, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks, const void* rings,
                               uint64_t rings_bytes, const void* socks_out, const void* payload, uint64_t payload_cap,
                               const void* runs, const void* order, const void* totals, bool aligned,
                               std::vector<uint32_t>& table, dl::Check& c) {
    const fs_status st =
        flows_check(ctx, fn, frames, offsets, lengths, n, flags, payload, payload_cap, runs, order, totals, aligned);
    if (st != FS_SUCCESS) return st;
    c = dl::check_socks(socks, n_socks, rings != nullptr, socks_out != nullptr, rings_bytes, ctx->flow_hash_mask, table);
    if (c.bad != dl::kGood)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": socket " + std::to_string(c.sock) + ": " + dl::bad_text(c.bad));
    return FS_SUCCESS;
}

// The launches of a checked device-resident delivery call on `stream`: the flow call's (or its zero
// totals for an empty batch), `delivered` zeroed, the socket block staged in a block of its own, the
// delivery kernels. `d_copied`: as coalesce_enqueue's (non-empty batches only). `layout` (nullable):
// flows_enqueue's, for the receive call's launches behind these.
static fs_status deliver_enqueue(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                 uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                                 const std::vector<uint32_t>& table, uint8_t* rings, fs_rx_sock_out* socks_out,
                                 uint8_t* delivered, uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs,
                                 fs_rx_flow* flows, uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals,
                                 fs_digest* out, uint8_t* status, hipStream_t stream, const uint8_t** d_copied = nullptr,
                                 framesum::FlowScratch* layout = nullptr) {
    framesum::FlowScratch fs{};
    if (n == 0) {
        FS_HIP(ctx, hipMemsetAsync(totals, 0, sizeof(fs_rx_flow_totals), stream));
    } else {
        const fs_status st = flows_enqueue(ctx, frames, offsets, lengths, n, mtu, flags, payload, payload_cap, runs, flows,
                                           order, run_of, totals, out, status, stream, d_copied, &fs);
        if (st != FS_SUCCESS) return st;
        if (delivered) FS_HIP(ctx, hipMemsetAsync(delivered, 0, n, stream));
    }
    if (layout) *layout = fs;
    if (n_socks == 0) return FS_SUCCESS;
    const dl::Block b = dl::block_of(n_socks);
    const framesum::DeliverScratch ds = framesum::deliver_scratch(n, n_socks);
    fs_status st = ctx->dl_scratch.grow(ctx, ds.bytes);
    if (st != FS_SUCCESS) return st;
    SegStage* sg = nullptr;
    st = stage_block(ctx, b.bytes, &sg);
    if (st != FS_SUCCESS) return st;
    std::memcpy(sg->h, socks, b.table);
    std::memcpy(sg->h + b.table, table.data(), 4ull * table.size());
    FS_HIP(ctx, hipMemcpyAsync(sg->d, sg->h, b.bytes, hipMemcpyHostToDevice, stream));
    sg->used = true;  // (from here on the block may be read by queued work)
    const int wgs = ctx->workgroups > 0 ? ctx->workgroups : 8 * ctx->num_cus;
    const hipError_t le = framesum::launch_deliver(frames, offsets, n, ctx->fl_scratch.p, fs, totals, sg->d, n_socks,
                                                   ctx->flow_hash_mask, rings, socks_out, delivered, ctx->dl_scratch.p, ds,
                                                   wgs, stream);
    const hipError_t re = hipEventRecord(sg->done, stream);
    if (le != hipSuccess) return hip_err(ctx, le, "fs_deliver_flows_batch: launch");
    if (re != hipSuccess) return hip_err(ctx, re, "hipEventRecord(sg->done, stream)");
    return FS_SUCCESS;
}

fs_status fs_deliver_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                 uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                                 uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                                 uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows,
                                 uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out,
                                 uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    std::vector<uint32_t> table;
    dl::Check c;
    const fs_status st = deliver_check(ctx, "fs_deliver_flows_batch", frames, offsets, lengths, n, flags, socks, n_socks, rings,
                                       rings_bytes, socks_out, payload, payload_cap, runs, order, totals, true, table, c);
    if (st != FS_SUCCESS) return st;
    FS_HIP(ctx, hipSetDevice(ctx->device));
    return deliver_enqueue(ctx, frames, offsets, lengths, n, mtu, flags, socks, n_socks, table, rings, socks_out, delivered,
                           payload, payload_cap, runs, flows, order, run_of, totals, out, status,
                           reinterpret_cast<hipStream_t>(stream));
}

// ---- The receive call (fs_recv_flows_batch / fs_recv_flows_batch_host, include/framesum_recv.h): the
// delivery, and behind it the fold of every listed socket's ACKs and windows (framesum_recv.hip) ----

namespace rv = framesum::recv;

// What the receive call adds to the delivery's arguments.
struct RecvPart {
    const fs_rx_snd* snd;
    fs_rx_snd_out* snd_out;
    uint8_t* code;
};

static fs_status recv_check(fs_ctx* ctx, const char* fn, const fs_rx_sock* socks, uint32_t n_socks, const RecvPart& rp) {
    const rv::CheckSnd c = rv::check_snd(socks, rp.snd, n_socks, rp.snd_out != nullptr);
    if (c.bad != rv::kSndGood)
        return set_err(ctx, FS_E_INVALID, std::string(fn) + ": socket " + std::to_string(c.sock) + ": " + rv::bad_snd_text(c.bad));
    return FS_SUCCESS;
}

// The launches of a checked device-resident receive call on `stream`: deliver_enqueue's, `code`
// zeroed, the send-side block staged in a block of its own, the receive kernels.
static fs_status recv_enqueue(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                              uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                              const std::vector<uint32_t>& table, uint8_t* rings, fs_rx_sock_out* socks_out,
                              uint8_t* delivered, const RecvPart& rp, uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs,
                              fs_rx_flow* flows, uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out,
                              uint8_t* status, hipStream_t stream, const uint8_t** d_copied = nullptr) {
    framesum::FlowScratch fs{};
    fs_status st = deliver_enqueue(ctx, frames, offsets, lengths, n, mtu, flags, socks, n_socks, table, rings, socks_out,
                                   delivered, payload, payload_cap, runs, flows, order, run_of, totals, out, status, stream,
                                   d_copied, &fs);
    if (st != FS_SUCCESS) return st;
    if (rp.code && n != 0) FS_HIP(ctx, hipMemsetAsync(rp.code, 0, n, stream));
    if (n_socks == 0) return FS_SUCCESS;
    const framesum::RecvScratch rs = framesum::recv_scratch(n);
    st = ctx->rv_scratch.grow(ctx, rs.bytes);
    if (st != FS_SUCCESS) return st;
    const uint64_t block_bytes = (uint64_t)n_socks * sizeof(rv::Sock);
    SegStage* sg = nullptr;
    st = stage_block(ctx, block_bytes, &sg);
    if (st != FS_SUCCESS) return st;
    rv::stage(socks, rp.snd, n_socks, reinterpret_cast<rv::Sock*>(sg->h));
    FS_HIP(ctx, hipMemcpyAsync(sg->d, sg->h, block_bytes, hipMemcpyHostToDevice, stream));
    sg->used = true;  // (from here on the block may be read by queued work)
    const int wgs = ctx->workgroups > 0 ? ctx->workgroups : 8 * ctx->num_cus;
    const hipError_t le = framesum::launch_recv(frames, offsets, n, ctx->fl_scratch.p, fs, ctx->dl_scratch.p,
                                                framesum::deliver_scratch(n, n_socks), socks_out, sg->d, n_socks, rp.snd_out,
                                                rp.code, ctx->rv_scratch.p, rs, wgs, stream);
    const hipError_t re = hipEventRecord(sg->done, stream);
    if (le != hipSuccess) return hip_err(ctx, le, "fs_recv_flows_batch: launch");
    if (re != hipSuccess) return hip_err(ctx, re, "hipEventRecord(sg->done, stream)");
    return FS_SUCCESS;
}

// The host form of the delivery (`rp` null) and of the receive call, behind their checks.
static fs_status deliver_host(fs_ctx* ctx, const char* fn, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                              const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks,
                              uint32_t n_socks, const std::vector<uint32_t>& table, const dl::Check& c, uint8_t* rings,
                              fs_rx_sock_out* socks_out, uint8_t* delivered, const RecvPart* rp, uint8_t* payload,
                              uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                              fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status) {
    if (n == 0) {  // nothing for a device to do: the sockets keep their state
        std::memset(totals, 0, sizeof(fs_rx_flow_totals));
        for (uint32_t s = 0; s < n_socks; ++s) socks_out[s] = dl::untouched(socks[s]);
        for (uint32_t s = 0; rp && s < n_socks; ++s) rp->snd_out[s] = rv::untouched(rp->snd[s].snd_una, rp->snd[s].snd_wnd);
        return FS_SUCCESS;
    }
    // the device's socks_out (and snd_out behind it) and the rings' span (the kernels address ring bytes
    // at base + ring_off)
    const uint64_t span = c.hi - c.lo;
    const uint64_t at_snd_out = (uint64_t)n_socks * sizeof(fs_rx_sock_out);
    fs_status st = begin_host_call(ctx);
    if (st == FS_SUCCESS) st = ctx->dl_arrays.grow(ctx, at_snd_out + (rp ? (uint64_t)n_socks * sizeof(fs_rx_snd_out) : 0));
    if (st == FS_SUCCESS) st = ctx->dl_rings.grow(ctx, span);
    if (st != FS_SUCCESS) return st;
    fs_rx_sock_out* d_socks_out = ctx->dl_arrays.as<fs_rx_sock_out>();
    fs_rx_snd_out* d_snd_out = ctx->dl_arrays.as<fs_rx_snd_out>(at_snd_out);
    uint8_t* d_rings = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(ctx->dl_rings.p) - c.lo);
    // behind the runs, per frame: a flow (32), order (4), run_of (4), delivered (1), code (1, the receive call)
    const uint64_t at_order = (uint64_t)n * 32, at_run_of = (uint64_t)n * 36, at_delivered = (uint64_t)n * 40,
                   at_code = (uint64_t)n * 41;
    return rx_host(
        ctx, fn, frames, frames_bytes, offsets, lengths, n, payload, payload_cap, runs, totals, out, status, ctx->fl_arrays,
        rp ? 42 : 41,
        [&](const Staged& s, uint64_t d_cap, fs_rx_run* d_runs, uint8_t* d_rest, fs_rx_flow_totals* d_totals,
            const uint8_t** d_copied) {
            // the span goes in first, so that the copy back returns the caller's own bytes between the rings
            if (span != 0) FS_HIP(ctx, hipMemcpyAsync(ctx->dl_rings.p, rings + c.lo, span, hipMemcpyHostToDevice, s.ks));
            uint8_t* d_delivered = delivered ? d_rest + at_delivered : nullptr;
            fs_rx_flow* d_flows = flows ? reinterpret_cast<fs_rx_flow*>(d_rest) : nullptr;
            uint32_t* d_order = reinterpret_cast<uint32_t*>(d_rest + at_order);
            uint32_t* d_run_of = run_of ? reinterpret_cast<uint32_t*>(d_rest + at_run_of) : nullptr;
            if (!rp)
                return deliver_enqueue(ctx, s.base, s.d_off, s.d_len, n, mtu, flags, socks, n_socks, table, d_rings, d_socks_out,
                                       d_delivered, ctx->co_payload.p, d_cap, d_runs, d_flows, d_order, d_run_of, d_totals,
                                       s.d_out, s.d_st, s.ks, d_copied);
            const RecvPart d_rp{rp->snd, d_snd_out, rp->code ? d_rest + at_code : nullptr};
            return recv_enqueue(ctx, s.base, s.d_off, s.d_len, n, mtu, flags, socks, n_socks, table, d_rings, d_socks_out,
                                d_delivered, d_rp, ctx->co_payload.p, d_cap, d_runs, d_flows, d_order, d_run_of, d_totals,
                                s.d_out, s.d_st, s.ks, d_copied);
        },
        [&](const fs_rx_flow_totals& t) { return t.n_accepted <= n && t.n_runs <= t.n_accepted && t.n_flows <= t.n_runs; },
        [&](const fs_rx_flow_totals& t, const uint8_t* d_rest) {
            return std::array<D2H, 8>{{{flows, d_rest, (uint64_t)t.n_flows * sizeof(fs_rx_flow)},
                                       {order, d_rest + at_order, (uint64_t)t.n_accepted * 4},
                                       {run_of, d_rest + at_run_of, (uint64_t)n * 4},
                                       {delivered, d_rest + at_delivered, (uint64_t)n},
                                       {n_socks ? rings + c.lo : nullptr, ctx->dl_rings.p, span},
                                       {socks_out, d_socks_out, (uint64_t)n_socks * sizeof(fs_rx_sock_out)},
                                       {rp ? rp->snd_out : nullptr, d_snd_out, (uint64_t)n_socks * sizeof(fs_rx_snd_out)},
                                       {rp ? rp->code : nullptr, d_rest + at_code, (uint64_t)n}}};
        });
}

fs_status fs_deliver_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                      const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                      const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                      fs_rx_sock_out* socks_out, uint8_t* delivered, uint8_t* payload,
                                      uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                                      uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    const char* const fn = "fs_deliver_flows_batch_host";
    std::vector<uint32_t> table;
    dl::Check c;
    const fs_status ast = deliver_check(ctx, fn, frames, offsets, lengths, n, flags, socks, n_socks, rings, rings_bytes,
                                        socks_out, payload, payload_cap, runs, order, totals, false, table, c);
    if (ast != FS_SUCCESS) return ast;
    return deliver_host(ctx, fn, frames, frames_bytes, offsets, lengths, n, mtu, flags, socks, n_socks, table, c, rings,
                        socks_out, delivered, nullptr, payload, payload_cap, runs, flows, order, run_of, totals, out, status);
}

fs_status fs_recv_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                              uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                              uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                              const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, uint8_t* payload,
                              uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                              uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    const char* const fn = "fs_recv_flows_batch";
    std::vector<uint32_t> table;
    dl::Check c;
    const RecvPart rp{snd, snd_out, code};
    fs_status st = deliver_check(ctx, fn, frames, offsets, lengths, n, flags, socks, n_socks, rings, rings_bytes, socks_out,
                                 payload, payload_cap, runs, order, totals, true, table, c);
    if (st == FS_SUCCESS) st = recv_check(ctx, fn, socks, n_socks, rp);
    if (st != FS_SUCCESS) return st;
    FS_HIP(ctx, hipSetDevice(ctx->device));
    return recv_enqueue(ctx, frames, offsets, lengths, n, mtu, flags, socks, n_socks, table, rings, socks_out, delivered, rp,
                        payload, payload_cap, runs, flows, order, run_of, totals, out, status,
                        reinterpret_cast<hipStream_t>(stream));
}

fs_status fs_recv_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                   const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                   const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                   fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                   fs_rx_snd_out* snd_out, uint8_t* code, uint8_t* payload, uint64_t payload_cap,
                                   fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                   fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    const char* const fn = "fs_recv_flows_batch_host";
    std::vector<uint32_t> table;
    dl::Check c;
    const RecvPart rp{snd, snd_out, code};
    fs_status ast = deliver_check(ctx, fn, frames, offsets, lengths, n, flags, socks, n_socks, rings, rings_bytes, socks_out,
                                  payload, payload_cap, runs, order, totals, false, table, c);
    if (ast == FS_SUCCESS) ast = recv_check(ctx, fn, socks, n_socks, rp);
    if (ast != FS_SUCCESS) return ast;
    return deliver_host(ctx, fn, frames, frames_bytes, offsets, lengths, n, mtu, flags, socks, n_socks, table, c, rings,
                        socks_out, delivered, &rp, payload, payload_cap, runs, flows, order, run_of, totals, out, status);
}
