// framesum C ABI (include/framesum.h) -- the two RX coalesce families: fs_coalesce_batch and
// fs_coalesce_batch_host (kernels: framesum_coalesce.hip), fs_coalesce_flows_batch and
// fs_coalesce_flows_batch_host (framesum_flows.hip), and what their host forms share.
#include <algorithm>
#include <array>
#include <cstring>
#include <string>

#include "framesum_ctx.h"
#include "framesum_flows.h"

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
// `stream`. `d_copied`: as coalesce_enqueue's.
static fs_status flows_enqueue(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                               uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                               fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                               fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, hipStream_t stream,
                               const uint8_t** d_copied = nullptr) {
    const framesum::FlowScratch s = framesum::flows_scratch(n);
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
