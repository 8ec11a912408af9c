// framesum C ABI -- the nine RX call kinds, each with a device form and a host form:
//   the plain coalesce       fs_coalesce_batch, fs_coalesce_batch_host (include/framesum.h;
//                            kernels: framesum_coalesce.hip)
//   the flow-aware coalesce  fs_coalesce_flows_batch, ..._host (framesum_flows.hip)
//   the delivery             fs_deliver_flows_batch, ..._host (include/framesum_deliver.h;
//                            framesum_deliver.hip): the flow call, then the delivery into socket rings
//   the receive call         fs_recv_flows_batch, ..._host (include/framesum_recv.h; framesum_recv.hip):
//                            the delivery, then the fold of every listed socket's ACKs and windows
//   the accept call          fs_accept_flows_batch, ..._host (include/framesum_accept.h;
//                            framesum_accept.hip): the receive call, then the passive open of every first
//                            SYN to a listener, with its SYN-ACK
//   the close call           fs_close_flows_batch, ..._host (include/framesum_close.h;
//                            framesum_close.hip): the accept call, then the control walks of the closing
//                            states and of an RST
//   the connect call         fs_connect_flows_batch, ..._host (include/framesum_connect.h;
//                            framesum_connect.hip): the close call, then the active open of every listed
//                            opener, with the control frame it owes
//   the UDP call             fs_udp_flows_batch, ..._host (include/framesum_udp.h; framesum_udp.hip): the
//                            connect call, then every accepted UDP frame into its port's queue of cells
//   the ARP call             fs_arp_flows_batch, ..._host (include/framesum_arp.h; framesum_arp.hip): the
//                            UDP call, then every ARP request answered and every ARP reply matched
// A call is one record (RxCall) that the entry point fills from its flat arguments; the checks, the
// stages up to the call's kind and the one host form all read that record.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "framesum_accept.h"
#include "framesum_close.h"
#include "framesum_connect.h"
#include "framesum_ctx.h"
#include "framesum_deliver.h"
#include "framesum_flows.h"
#include "framesum_recv.h"
#include "framesum_udp.h"
#include "framesum_arp.h"

using namespace framesum::host;
using framesum::RxBatch;
using framesum::RxLaunch;
using framesum::RxLeft;
using framesum::RxResults;
namespace rxp = framesum::plan::rx;
namespace dl = framesum::deliver;
namespace rv = framesum::recv;
namespace ac = framesum::accept;
namespace cl = framesum::closing;
namespace cn = framesum::connect;
namespace ud = framesum::udp;
namespace ar = framesum::arp;

namespace {

// A list of an accept, a close or a connect call: the caller's records, where the call's own results go (`dev`:
// the caller's pointers, host or device as the form has them, with the list's counts), and the table the list's
// check builds. l: the listeners (with their second list, the slots), k: the closers, o: the openers.
template <class Rec, class Dev>
struct RxList {
    const Rec* recs = nullptr;
    Dev dev{};
    std::vector<uint32_t> table;
};
struct RxListen : RxList<fs_listener, framesum::RxAccept> {
    const fs_accept_slot* slots = nullptr;
};
using RxClosing = RxList<fs_cl_sock, framesum::RxClose>;
using RxOpening = RxList<fs_cn_sock, framesum::RxConnect>;
// The port list of a UDP call, with what its check makes of it (the span of `cells` the queues cover).
struct RxPorts : RxList<fs_udp_port, framesum::RxUdp> {
    uint64_t cells_bytes = 0;
    ud::CheckUdp span{};
};

// The host and query lists of an ARP call, with what their check builds (the key records and the tables).
struct RxNeighbours {
    const fs_arp_host* hosts = nullptr;
    const fs_arp_query* queries = nullptr;
    framesum::RxArp dev{};
    ar::Built built;
};

// The socket part of a delivery or a receive call: the caller's lists, and what check_socks makes of
// them (the socket table, the span of `rings` the listed rings cover).
struct RxSocks {
    const fs_rx_sock* socks = nullptr;
    const fs_rx_snd* snd = nullptr;
    uint32_t n_socks = 0;
    uint64_t rings_bytes = 0;
    std::vector<uint32_t> table;
    dl::Check span{};
};
// A call as its entry point got it: `fn` names it in the error texts, `r` holds the caller's pointers.
struct RxCall {
    rxp::Kind kind;
    const char* fn;
    RxBatch b;
    RxResults r{};
    RxSocks s;
    RxListen l;
    RxClosing k;
    RxOpening o;
    RxPorts p;
    RxNeighbours a;
    RxCall(rxp::Kind kind_, const char* fn_, const RxBatch& b_) : kind(kind_), fn(fn_), b(b_) {}
    // the flat arguments, group by group as the ABI lists them
    void coalesce(uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, uint32_t* run_of, void* totals, fs_digest* out,
                  uint8_t* status) {
        r.payload = payload, r.payload_cap = payload_cap, r.out = out, r.status = status;
        r.array[rxp::kRuns] = runs, r.array[rxp::kRunOf] = run_of, r.array[rxp::kTotals] = totals;
    }
    void flows(fs_rx_flow* flows, uint32_t* order) { r.array[rxp::kFlowRecs] = flows, r.array[rxp::kOrder] = order; }
    void sockets(const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out,
                 uint8_t* delivered) {
        s.socks = socks, s.n_socks = n_socks, s.rings_bytes = rings_bytes, r.rings = rings;
        r.array[rxp::kSocksOut] = socks_out, r.array[rxp::kDelivered] = delivered;
    }
    void send_side(const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code) {
        s.snd = snd, r.array[rxp::kSndOut] = snd_out, r.array[rxp::kCode] = code;
    }
    void listening(const fs_listener* listeners, uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                   uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                   uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status) {
        l.recs = listeners, l.slots = slots;
        l.dev = framesum::RxAccept{s.n_socks, n_listeners, n_slots, synack_flags, conns, listeners_out,
                                 accept_of,  synacks,     synack_out, synack_status};
    }
    void closing(const fs_cl_sock* closers, uint32_t n_closers, fs_cl_out* closers_out, fs_cl_out* socks_close,
                 uint8_t* ctl_code) {
        k.recs = closers;
        k.dev = framesum::RxClose{s.n_socks, n_closers, closers_out, socks_close, ctl_code};
    }
    void opening(const fs_cn_sock* openers, uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out, uint8_t* replies,
                 fs_digest* reply_out, uint8_t* reply_status) {
        o.recs = openers;
        o.dev = framesum::RxConnect{n_openers, reply_flags, openers_out, replies, reply_out, reply_status, k.dev.ctl_code};
    }
    void datagrams(const fs_udp_port* ports, uint32_t n_ports, uint8_t* cells, uint64_t cells_bytes, fs_udp_port_out* ports_out,
                   uint32_t* port_of, uint32_t* cell_of) {
        p.recs = ports, p.cells_bytes = cells_bytes;
        p.dev = framesum::RxUdp{n_ports, 0u, cells, ports_out, port_of, cell_of};
    }
    void neighbours(const fs_arp_host* hosts, uint32_t n_hosts, const fs_arp_query* queries, uint32_t n_queries,
                    uint32_t n_reply_slots, uint32_t arp_flags, fs_arp_host_out* hosts_out, fs_arp_query_out* queries_out,
                    uint8_t* arp_frames, fs_digest* arp_out, uint8_t* arp_status, uint8_t* arp_code, uint32_t* arp_of) {
        a.hosts = hosts, a.queries = queries;
        a.dev = framesum::RxArp{n_hosts,    n_queries, n_reply_slots, arp_flags, hosts_out, queries_out,
                                arp_frames, arp_out,   arp_status,    arp_code,  arp_of};
    }
};
// The call as the launches see it: in the device forms the caller's batch and arrays on the caller's
// stream, in the host forms the staged batch and the context's device arrays on the compute stream.
struct RxDevice {
    RxBatch b;
    RxResults r;
    hipStream_t stream;
    framesum::RxAccept x{};  // (the accept call and the close call)
    framesum::RxClose y{};   // (the close call and the connect call)
    framesum::RxConnect z{}; // (the connect call and the UDP call)
    framesum::RxUdp u{};     // (the UDP call and the ARP call)
    framesum::RxArp w{};     // (the ARP call only)
};

fs_status invalid(fs_ctx* ctx, const RxCall& c, const std::string& what) {
    return set_err(ctx, FS_E_INVALID, std::string(c.fn) + ": " + what);
}

// Every check of a call, none of which needs a device; `aligned`: the device forms' alignment of
// `frames`. An empty batch needs only `totals` and, in the socket calls, good sockets.
fs_status rx_check(fs_ctx* ctx, RxCall& c, bool aligned) {
    const RxBatch& b = c.b;
    const bool by_flow = c.kind != rxp::kPlain;
    if (by_flow && b.n > framesum::flows::kMaxFrames) return invalid(ctx, c, "n too large (at most 2^30 frames per call)");
    if (b.flags & ~(uint32_t)FS_RX_FCS) return invalid(ctx, c, "flags must be 0 or FS_RX_FCS");
    if (b.n > kMaxFrames) return invalid(ctx, c, "n too large (at most 2^31 frames per call)");
    if (!c.r.totals()) return invalid(ctx, c, "null pointer");
    if (b.n != 0) {
        if (!b.frames || !b.offsets || !b.lengths || !c.r.runs()) return invalid(ctx, c, "null pointer");
        if (!c.r.payload && c.r.payload_cap != 0) return invalid(ctx, c, "null payload with a non-zero payload_cap");
        if (aligned && (reinterpret_cast<uintptr_t>(b.frames) & 3u)) return invalid(ctx, c, "frames must be 4-byte aligned");
        if (by_flow && !c.r.order()) return invalid(ctx, c, "null pointer");  // (as `runs`)
    }
    if (c.kind >= rxp::kDeliver) {  // the socket list's checks (framesum_deliver.h), which also build the table
        RxSocks& s = c.s;
        s.span = dl::check_socks(s.socks, s.n_socks, c.r.rings != nullptr, c.r.socks_out() != nullptr, s.rings_bytes,
                                 ctx->flow_hash_mask, s.table);
        if (s.span.bad != dl::kGood)
            return invalid(ctx, c, "socket " + std::to_string(s.span.sock) + ": " + dl::bad_text(s.span.bad));
    }
    if (c.kind >= rxp::kRecv) {
        const rv::CheckSnd cs = rv::check_snd(c.s.socks, c.s.snd, c.s.n_socks, c.r.snd_out() != nullptr);
        if (cs.bad != rv::kSndGood) return invalid(ctx, c, "socket " + std::to_string(cs.sock) + ": " + rv::bad_snd_text(cs.bad));
    }
    if (c.kind >= rxp::kAccept) {  // the listener and slot lists' checks (framesum_accept.h), which also build the table
        RxListen& l = c.l;
        const ac::CheckAccept ca =
            ac::check_accept(l.recs, l.dev.n_listeners, l.slots, l.dev.n_slots, l.dev.synack_flags, l.dev.conns != nullptr,
                             l.dev.listeners_out != nullptr, l.dev.synacks != nullptr, ctx->flow_hash_mask, l.table);
        if (ca.bad != ac::kAcceptGood)
            return invalid(ctx, c, "listener or slot " + std::to_string(ca.index) + ": " + ac::bad_accept_text(ca.bad));
    }
    if (c.kind >= rxp::kClose) {  // the closer list's checks (framesum_close.h), which also build the table
        RxClosing& k = c.k;
        const cl::CheckClose cc =
            cl::check_closers(k.recs, k.dev.n_closers, k.dev.closers_out != nullptr, k.dev.socks_close != nullptr, c.s.socks,
                              c.s.n_socks, c.s.table.data(), ctx->flow_hash_mask, k.table);
        if (cc.bad != cl::kCloseGood)
            return invalid(ctx, c, "closer " + std::to_string(cc.index) + ": " + cl::bad_close_text(cc.bad));
    }
    if (c.kind >= rxp::kConnect) {  // the opener list's checks (framesum_connect.h), which also build the table
        RxOpening& o = c.o;
        const cn::CheckConnect co =
            cn::check_openers(o.recs, o.dev.n_openers, o.dev.reply_flags, o.dev.openers_out != nullptr, o.dev.replies != nullptr,
                              c.s.socks, c.s.n_socks, c.s.table.data(), c.k.recs, c.k.dev.n_closers, c.k.table.data(),
                              ctx->flow_hash_mask, o.table);
        if (co.bad != cn::kConnectGood)
            return invalid(ctx, c, "opener " + std::to_string(co.index) + ": " + cn::bad_connect_text(co.bad));
    }
    if (c.kind >= rxp::kUdp) {  // the port list's checks (framesum_udp.h), which also build the table
        RxPorts& p = c.p;
        p.span = ud::check_ports(p.recs, p.dev.n_ports, p.dev.cells != nullptr, p.dev.ports_out != nullptr, p.cells_bytes,
                                 ctx->flow_hash_mask, p.table);
        if (p.span.bad != ud::kUdpGood)
            return invalid(ctx, c, "port " + std::to_string(p.span.index) + ": " + ud::bad_udp_text(p.span.bad));
        p.dev.max_cell = ud::max_cell_size(p.recs, p.dev.n_ports);
    }
    if (c.kind == rxp::kArp) {  // the host and query lists' checks (framesum_arp.h), which also build the tables
        RxNeighbours& a = c.a;
        const ar::CheckArp ca = ar::check_arp(a.hosts, a.dev.n_hosts, a.queries, a.dev.n_queries, a.dev.n_reply_slots,
                                              a.dev.arp_flags, a.dev.hosts_out != nullptr, a.dev.queries_out != nullptr,
                                              a.dev.arp_frames != nullptr, ctx->flow_hash_mask, a.built);
        if (ca.bad != ar::kArpGood)
            return invalid(ctx, c, "host or query " + std::to_string(ca.index) + ": " + ar::bad_arp_text(ca.bad));
    }
    return FS_SUCCESS;
}

// ---- The stages of a checked call on the device. Each enqueues on d.stream behind the one before it.

// The cap of the grids behind the digest launch: up to 8 workgroups of 256 lanes per CU unless
// fs_ctx_set_workgroups caps them.
int rx_workgroups(const fs_ctx* ctx) { return ctx->workgroups > 0 ? ctx->workgroups : 8 * ctx->num_cus; }
// The cap of a control-frame kernel's grid (the SYN-ACKs, the replies) as the TX frame build has it: two
// workgroups per CU (their tables fit its LDS twice) unless fs_ctx_set_workgroups asks for fewer.
int tx_workgroups(const fs_ctx* ctx) {
    return ctx->workgroups > 0 && ctx->workgroups < 2 * ctx->num_cus ? ctx->workgroups : 2 * ctx->num_cus;
}

// `out` and `status` of a device-resident call that passes none: the context's own.
fs_status spare_results(fs_ctx* ctx, RxDevice& d) {
    if (d.r.out && d.r.status) return FS_SUCCESS;
    const fs_status st = ctx->co_results.grow(ctx, (uint64_t)d.b.n * 9);
    if (st != FS_SUCCESS) return st;
    if (!d.r.out) d.r.out = ctx->co_results.as<fs_digest>();
    if (!d.r.status) d.r.status = ctx->co_results.p + (uint64_t)d.b.n * 8;
    return FS_SUCCESS;
}

hipError_t digest_launch(fs_ctx* ctx, const RxDevice& d) {
    return launch(ctx, d.b.frames, d.b.offsets, d.b.lengths, d.b.n, d.b.mtu, d.r.out, d.r.status, d.stream,
                  (d.b.flags & FS_RX_FCS) ? framesum::FsOp::kFcs : framesum::FsOp::kDigest, nullptr, 0);
}

// The digest launch and the plain gather of a non-empty batch.
fs_status plain_stage(fs_ctx* ctx, RxDevice& d, const RxLaunch& how, RxLeft& left) {
    const framesum::CoScratch s = framesum::coalesce_scratch(d.b.n);
    fs_status st = ctx->co_scratch.grow(ctx, s.bytes);
    if (st == FS_SUCCESS) st = spare_results(ctx, d);
    if (st != FS_SUCCESS) return st;
    left.copied = ctx->co_scratch.p + s.copied;
    FS_HIP(ctx, digest_launch(ctx, d));
    FS_HIP(ctx, framesum::launch_coalesce(d.b, d.r, ctx->co_scratch.p, how));
    return FS_SUCCESS;
}

// The digest launch (skipped unless all of the flow launches' steps run: the test library's hook) and
// the flow gather of a non-empty batch.
fs_status flows_stage(fs_ctx* ctx, RxDevice& d, const RxLaunch& how, RxLeft& left) {
    left.fs = framesum::flows_scratch(d.b.n);
    if (left.fs.sort_bytes == 0)
        return set_err(ctx, FS_E_HIP, "fs_coalesce_flows_batch: the sort reports no temporary storage size");
    fs_status st = ctx->fl_scratch.grow(ctx, left.fs.bytes);
    if (st == FS_SUCCESS) st = spare_results(ctx, d);
    if (st != FS_SUCCESS) return st;
    left.flow_scratch = ctx->fl_scratch.p;
    left.copied = left.flow_scratch + left.fs.copied;
    if (how.steps == framesum::kFlowStepsAll) FS_HIP(ctx, digest_launch(ctx, d));
    FS_HIP(ctx, framesum::launch_coalesce_flows(d.b, d.r, left, how));
    return FS_SUCCESS;
}

// `delivered` zeroed, the socket block staged in a block of its own, the delivery kernels (which run
// for an empty batch too: the sockets' out records are written).
fs_status deliver_stage(fs_ctx* ctx, const RxSocks& s, const RxDevice& d, const RxLaunch& how, RxLeft& left) {
    if (d.b.n != 0 && d.r.delivered()) FS_HIP(ctx, hipMemsetAsync(d.r.delivered(), 0, d.b.n, d.stream));
    if (s.n_socks == 0) return FS_SUCCESS;
    const dl::Block blk = dl::block_of(s.n_socks);
    left.ds = framesum::deliver_scratch(d.b.n, s.n_socks);
    const fs_status st = ctx->dl_scratch.grow(ctx, left.ds.bytes);
    if (st != FS_SUCCESS) return st;
    left.deliver_scratch = ctx->dl_scratch.p;
    const auto fill = [&](uint8_t* h_block) {
        std::memcpy(h_block, s.socks, blk.table);
        std::memcpy(h_block + blk.table, s.table.data(), 4ull * s.table.size());
    };
    const auto kernels = [&](const uint8_t* d_block) { return framesum::launch_deliver(d.b, d.r, left, d_block, s.n_socks, how); };
    return staged_launch(ctx, blk.bytes, d.stream, "fs_deliver_flows_batch: launch", fill, kernels);
}

// `code` zeroed, the send-side block staged in a block of its own, the receive kernels.
fs_status recv_stage(fs_ctx* ctx, const RxSocks& s, const RxDevice& d, const RxLaunch& how, RxLeft& left) {
    if (d.b.n != 0 && d.r.code()) FS_HIP(ctx, hipMemsetAsync(d.r.code(), 0, d.b.n, d.stream));
    if (s.n_socks == 0) return FS_SUCCESS;
    left.rs = framesum::recv_scratch(d.b.n);
    const fs_status st = ctx->rv_scratch.grow(ctx, left.rs.bytes);
    if (st != FS_SUCCESS) return st;
    left.recv_scratch = ctx->rv_scratch.p;
    const auto fill = [&](uint8_t* h_block) { rv::stage(s.socks, s.snd, s.n_socks, reinterpret_cast<rv::Sock*>(h_block)); };
    const auto kernels = [&](const uint8_t* d_block) { return framesum::launch_recv(d.b, d.r, left, d_block, s.n_socks, how); };
    return staged_launch(ctx, (uint64_t)s.n_socks * sizeof(rv::Sock), d.stream, "fs_recv_flows_batch: launch", fill, kernels);
}

// `conns` and `listeners_out` zeroed and `accept_of` set to "none"; then, for a non-empty batch with
// listeners, the listener block staged in a block of its own and the accept kernels.
fs_status accept_stage(fs_ctx* ctx, const RxListen& l, const RxDevice& d, const RxLaunch& how, RxLeft& left) {
    const framesum::RxAccept& x = d.x;
    if (x.n_slots != 0) FS_HIP(ctx, hipMemsetAsync(x.conns, 0, (uint64_t)x.n_slots * sizeof(fs_accept_conn), d.stream));
    if (x.n_listeners != 0)
        FS_HIP(ctx, hipMemsetAsync(x.listeners_out, 0, (uint64_t)x.n_listeners * sizeof(fs_listener_out), d.stream));
    if (d.b.n != 0 && x.accept_of) FS_HIP(ctx, hipMemsetAsync(x.accept_of, 0xFF, 4ull * d.b.n, d.stream));
    if (d.b.n == 0 || x.n_listeners == 0) return FS_SUCCESS;
    left.acs = framesum::accept_scratch(d.b.n, x.n_listeners, x.n_slots);
    if (left.acs.sort_bytes == 0)
        return set_err(ctx, FS_E_HIP, "fs_accept_flows_batch: the sort reports no temporary storage size");
    fs_status st = ctx->ac_scratch.grow(ctx, left.acs.bytes);
    if (st == FS_SUCCESS) st = seg_tables(ctx);
    if (st != FS_SUCCESS) return st;
    left.accept_scratch = ctx->ac_scratch.p;
    const ac::Block blk = ac::block_of(x.n_listeners, x.n_slots);
    const auto fill = [&](uint8_t* h_block) {
        ac::stage(l.recs, x.n_listeners, l.table.data(), l.slots, x.n_slots, blk, h_block);
    };
    const auto kernels = [&](const uint8_t* d_block) {
        return framesum::launch_accept(d.b, x, left, d_block, ctx->d_seg_tables, tx_workgroups(ctx), how);
    };
    return staged_launch(ctx, blk.bytes, d.stream, "fs_accept_flows_batch: launch", fill, kernels);
}

// `ctl_code` zeroed; then, with a closer or a socket listed, the closers, their table and the sockets'
// fixed values staged in a block of their own and the close kernels (which run for an empty batch too:
// the out records are written).
fs_status close_stage(fs_ctx* ctx, const RxCall& c, const RxDevice& d, const RxLaunch& how, RxLeft& left) {
    const framesum::RxClose& y = d.y;
    if (d.b.n != 0 && y.ctl_code) FS_HIP(ctx, hipMemsetAsync(y.ctl_code, 0, d.b.n, d.stream));
    if (y.n_closers == 0 && y.n_socks == 0) return FS_SUCCESS;
    left.cs = framesum::owner_scratch(d.b.n, y.n_closers);
    const fs_status st = ctx->cl_scratch.grow(ctx, left.cs.bytes);
    if (st != FS_SUCCESS) return st;
    left.close_scratch = ctx->cl_scratch.p;
    const cl::Block blk = cl::block_of(y.n_closers, y.n_socks);
    const auto fill = [&](uint8_t* h_block) {
        cl::stage(c.k.recs, y.n_closers, c.k.table.data(), c.s.socks, y.n_socks, blk, h_block);
    };
    const auto kernels = [&](const uint8_t* d_block) { return framesum::launch_close(d.b, d.r, y, left, d_block, how); };
    return staged_launch(ctx, blk.bytes, d.stream, "fs_close_flows_batch: launch", fill, kernels);
}

// With an opener listed: the openers and their table staged in a block of their own and the connect
// kernels (which run for an empty batch too: the out records and the flagged SYNs are written).
fs_status connect_stage(fs_ctx* ctx, const RxCall& c, const RxDevice& d, const RxLaunch& how, RxLeft& left) {
    const framesum::RxConnect& z = d.z;
    if (z.n_openers == 0) return FS_SUCCESS;
    left.cns = framesum::connect_scratch(d.b.n, z.n_openers);
    fs_status st = ctx->cn_scratch.grow(ctx, left.cns.bytes);
    if (st == FS_SUCCESS) st = seg_tables(ctx);
    if (st != FS_SUCCESS) return st;
    left.connect_scratch = ctx->cn_scratch.p;
    const cn::Block blk = cn::block_of(z.n_openers);
    const auto fill = [&](uint8_t* h_block) { cn::stage(c.o.recs, z.n_openers, c.o.table.data(), blk, h_block); };
    const auto kernels = [&](const uint8_t* d_block) {
        return framesum::launch_connect(d.b, d.r, z, left, d_block, ctx->d_seg_tables, tx_workgroups(ctx), how);
    };
    return staged_launch(ctx, blk.bytes, d.stream, "fs_connect_flows_batch: launch", fill, kernels);
}

// `cell_of` set to "none", and `port_of` where no port is listed (the mark launch writes every entry
// otherwise); then, with a port listed, the ports and their table staged in a
// block of their own and the UDP kernels (which run for an empty batch too: the out records are written).
fs_status udp_stage(fs_ctx* ctx, const RxCall& c, const RxDevice& d, const RxLaunch& how, RxLeft& left) {
    const framesum::RxUdp& u = d.u;
    if (d.b.n != 0 && u.port_of && u.n_ports == 0) FS_HIP(ctx, hipMemsetAsync(u.port_of, 0xFF, 4ull * d.b.n, d.stream));
    if (d.b.n != 0 && u.cell_of) FS_HIP(ctx, hipMemsetAsync(u.cell_of, 0xFF, 4ull * d.b.n, d.stream));
    if (u.n_ports == 0) return FS_SUCCESS;
    left.us = framesum::udp_scratch(d.b.n, u.n_ports);
    if (d.b.n != 0 && left.us.sort_bytes == 0)
        return set_err(ctx, FS_E_HIP, "fs_udp_flows_batch: the sort reports no temporary storage size");
    const fs_status st = ctx->ud_scratch.grow(ctx, left.us.bytes);
    if (st != FS_SUCCESS) return st;
    left.udp_scratch = ctx->ud_scratch.p;
    const ud::Block blk = ud::block_of(u.n_ports);
    const auto fill = [&](uint8_t* h_block) { ud::stage(c.p.recs, u.n_ports, c.p.table.data(), blk, h_block); };
    const auto kernels = [&](const uint8_t* d_block) { return framesum::launch_udp(d.b, d.r, u, left, d_block, how); };
    return staged_launch(ctx, blk.bytes, d.stream, "fs_udp_flows_batch: launch", fill, kernels);
}

// With a host listed: the hosts, the queries and their tables staged in a block of their own and the ARP
// kernels (which run for an empty batch too: the out records and the flagged requests are written). With
// none: the one launch that writes `arp_code` and `arp_of`, where given.
fs_status arp_stage(fs_ctx* ctx, const RxCall& c, const RxDevice& d, const RxLaunch& how, RxLeft& left) {
    const framesum::RxArp& w = d.w;
    if (w.n_hosts == 0) {
        if (d.b.n == 0 || (!w.arp_code && !w.arp_of)) return FS_SUCCESS;
        FS_HIP(ctx, framesum::launch_arp(d.b, d.r, w, left, nullptr, nullptr, 0, how));
        return FS_SUCCESS;
    }
    left.ars = framesum::arp_scratch(d.b.n, w.n_hosts, w.n_queries, w.n_reply_slots);
    if (d.b.n != 0 && left.ars.sort_bytes == 0)
        return set_err(ctx, FS_E_HIP, "fs_arp_flows_batch: the sort reports no temporary storage size");
    fs_status st = ctx->ar_scratch.grow(ctx, left.ars.bytes);
    if (st == FS_SUCCESS) st = seg_tables(ctx);
    if (st != FS_SUCCESS) return st;
    left.arp_scratch = ctx->ar_scratch.p;
    const ar::Block blk = ar::block_of(w.n_hosts, w.n_queries);
    const auto fill = [&](uint8_t* h_block) { ar::stage(c.a.hosts, w.n_hosts, c.a.queries, w.n_queries, c.a.built, blk, h_block); };
    const auto kernels = [&](const uint8_t* d_block) {
        return framesum::launch_arp(d.b, d.r, w, left, d_block, ctx->d_seg_tables, tx_workgroups(ctx), how);
    };
    return staged_launch(ctx, blk.bytes, d.stream, "fs_arp_flows_batch: launch", fill, kernels);
}

// The stages up to the call's kind. An empty batch has zero totals in place of its gather; the socket
// calls still run their walks then. `left`: what the stages left (`copied`: non-empty batches only).
fs_status rx_run(fs_ctx* ctx, const RxCall& c, RxDevice d, RxLeft& left) {
    const RxLaunch how{rx_workgroups(ctx), ctx->flow_hash_mask, ctx->flow_steps, d.stream};
    left = RxLeft{};
    fs_status st = FS_SUCCESS;
    if (d.b.n == 0)
        FS_HIP(ctx, hipMemsetAsync(d.r.totals(), 0, rxp::totals_bytes(c.kind), d.stream));
    else
        st = c.kind == rxp::kPlain ? plain_stage(ctx, d, how, left) : flows_stage(ctx, d, how, left);
    if (st == FS_SUCCESS && c.kind >= rxp::kDeliver) st = deliver_stage(ctx, c.s, d, how, left);
    if (st == FS_SUCCESS && c.kind >= rxp::kRecv) st = recv_stage(ctx, c.s, d, how, left);
    if (st == FS_SUCCESS && c.kind >= rxp::kAccept) st = accept_stage(ctx, c.l, d, how, left);
    if (st == FS_SUCCESS && c.kind >= rxp::kClose) st = close_stage(ctx, c, d, how, left);
    if (st == FS_SUCCESS && c.kind >= rxp::kConnect) st = connect_stage(ctx, c, d, how, left);
    if (st == FS_SUCCESS && c.kind >= rxp::kUdp) st = udp_stage(ctx, c, d, how, left);
    if (st == FS_SUCCESS && c.kind == rxp::kArp) st = arp_stage(ctx, c, d, how, left);
    return st;
}

// A checked device form: the caller's pointers, on the caller's stream.
fs_status rx_device(fs_ctx* ctx, const RxCall& c, void* stream) {
    FS_HIP(ctx, hipSetDevice(ctx->device));
    RxLeft left;
    return rx_run(ctx, c, RxDevice{c.b, c.r, reinterpret_cast<hipStream_t>(stream), c.l.dev, c.k.dev, c.o.dev, c.p.dev, c.a.dev},
                  left);
}

// ---- The own arrays of the accept, the close and the connect call in a host form, walked by
// plan::rx::kExtraArrayDesc. `h`: the caller's host pointers in that table's order (null: the caller passed none).
struct RxExtra {
    void* h[rxp::kExtraArrays];
    void* d[rxp::kExtraArrays] = {};  // the device arrays, null where the call has none or the caller passed none
    rxp::ExtraLayout L{};
    explicit RxExtra(const RxCall& c)
        : h{c.l.dev.conns,       c.l.dev.listeners_out, c.l.dev.accept_of, c.l.dev.synacks,     c.l.dev.synack_out,
            c.l.dev.synack_status, c.k.dev.closers_out, c.k.dev.socks_close, c.k.dev.ctl_code, c.o.dev.openers_out,
            c.o.dev.replies,     c.o.dev.reply_out,     c.o.dev.reply_status} {}
    template <class T>
    T* as(rxp::ExtraArray a) const { return static_cast<T*>(d[a]); }
};
// The rows e.L lays out, carved from the context's buffer, which has room for them. Those of which the call writes some entries only go in first, so that the whole array comes back with the caller's bytes
// elsewhere.
fs_status extra_in(fs_ctx* ctx, RxExtra& e, hipStream_t ks) {
    for (uint32_t a = 0; a < rxp::kExtraArrays; ++a) {
        if (!e.h[a] || e.L.room[a] == 0) continue;
        e.d[a] = ctx->rx_arrays.p + e.L.at[a];
        if (rxp::kExtraArrayDesc[a].goes_in)
            FS_HIP_DRAIN(ctx, hipMemcpyAsync(e.d[a], e.h[a], e.L.room[a], hipMemcpyHostToDevice, ks));
    }
    return FS_SUCCESS;
}
fs_status extra_back(fs_ctx* ctx, const RxExtra& e, hipStream_t ks) {
    for (uint32_t a = 0; a < rxp::kExtraArrays; ++a)
        if (e.d[a]) FS_HIP_DRAIN(ctx, hipMemcpyAsync(e.h[a], e.d[a], e.L.room[a], hipMemcpyDeviceToHost, ks));
    return FS_SUCCESS;
}
rxp::ExtraCounts extra_counts(const RxCall& c) {
    return rxp::ExtraCounts{{c.l.dev.n_slots, c.l.dev.n_listeners, c.k.dev.n_closers, c.s.n_socks, c.o.dev.n_openers, c.b.n}};
}
// The three calls' parts as the launches of a host form see them: the counts, and the carved arrays.
framesum::RxAccept accept_device(const framesum::RxAccept& hx, const RxExtra& e) {
    return framesum::RxAccept{hx.n_socks, hx.n_listeners, hx.n_slots, hx.synack_flags, e.as<fs_accept_conn>(rxp::kConns),
                              e.as<fs_listener_out>(rxp::kListenersOut), e.as<uint32_t>(rxp::kAcceptOf),
                              e.as<uint8_t>(rxp::kSynacks), e.as<fs_digest>(rxp::kSynackOut), e.as<uint8_t>(rxp::kSynackStatus)};
}
framesum::RxClose close_device(const framesum::RxClose& hy, const RxExtra& e) {
    return framesum::RxClose{hy.n_socks, hy.n_closers, e.as<fs_cl_out>(rxp::kClosersOut), e.as<fs_cl_out>(rxp::kSocksClose),
                             e.as<uint8_t>(rxp::kCtlCode)};
}
framesum::RxConnect connect_device(const framesum::RxConnect& hz, const RxExtra& e) {
    return framesum::RxConnect{hz.n_openers, hz.reply_flags, e.as<fs_cn_out>(rxp::kOpenersOut), e.as<uint8_t>(rxp::kReplies),
                               e.as<fs_digest>(rxp::kReplyOut), e.as<uint8_t>(rxp::kReplyStatus), e.as<uint8_t>(rxp::kCtlCode)};
}

// The connect call's host form without a batch: nothing is staged but the openers; the connect stage alone
// runs on the compute stream over the context's device arrays, and its arrays come back.
fs_status connect_host_empty(fs_ctx* ctx, const RxCall& c) {
    RxExtra e(c);
    e.L = rxp::extra_layout(rxp::kConnect, rxp::kConnect, 0, extra_counts(c));
    fs_status st = begin_host_call(ctx);
    if (st == FS_SUCCESS) st = ctx->rx_arrays.grow(ctx, e.L.bytes);
    if (st != FS_SUCCESS) return st;
    const hipStream_t ks = ctx->compute_stream;
    ctx->host_dirty = true;
    st = extra_in(ctx, e, ks);
    if (st != FS_SUCCESS) return st;
    RxDevice d{c.b, RxResults{}, ks};
    d.z = connect_device(c.o.dev, e);
    const RxLaunch how{rx_workgroups(ctx), ctx->flow_hash_mask, ctx->flow_steps, ks};
    RxLeft left{};
    st = connect_stage(ctx, c, d, how, left);
    if (st != FS_SUCCESS) {
        drain_host_streams(ctx);
        return st;
    }
    st = extra_back(ctx, e, ks);
    if (st != FS_SUCCESS) return st;
    FS_HIP_DRAIN(ctx, hipStreamSynchronize(ks));
    ctx->host_dirty = false;
    return FS_SUCCESS;
}

// ---- The own arrays of the ARP call in a host form, walked by plan::rx::kArpArrayDesc.
struct RxArpArrays {
    void* h[rxp::kArpArrays];
    void* d[rxp::kArpArrays] = {};
    rxp::ArpLayout L{};
    explicit RxArpArrays(const framesum::RxArp& w)
        : h{w.hosts_out, w.queries_out, w.arp_frames, w.arp_out, w.arp_status, w.arp_code, w.arp_of} {}
    template <class T>
    T* as(rxp::ArpArray a) const { return static_cast<T*>(d[a]); }
};
rxp::ArpCounts arp_counts(const framesum::RxArp& w, uint64_t n) {
    return rxp::ArpCounts{{w.n_hosts, w.n_queries, (uint64_t)w.n_reply_slots + w.n_queries, n}};
}
fs_status arp_in(fs_ctx* ctx, RxArpArrays& e, hipStream_t ks) {
    for (uint32_t a = 0; a < rxp::kArpArrays; ++a) {
        if (!e.h[a] || e.L.room[a] == 0) continue;
        e.d[a] = ctx->rx_arrays.p + e.L.at[a];
        if (rxp::kArpArrayDesc[a].goes_in) FS_HIP_DRAIN(ctx, hipMemcpyAsync(e.d[a], e.h[a], e.L.room[a], hipMemcpyHostToDevice, ks));
    }
    return FS_SUCCESS;
}
fs_status arp_back(fs_ctx* ctx, const RxArpArrays& e, hipStream_t ks) {
    for (uint32_t a = 0; a < rxp::kArpArrays; ++a)
        if (e.d[a]) FS_HIP_DRAIN(ctx, hipMemcpyAsync(e.h[a], e.d[a], e.L.room[a], hipMemcpyDeviceToHost, ks));
    return FS_SUCCESS;
}
framesum::RxArp arp_device(const framesum::RxArp& hw, const RxArpArrays& e) {
    return framesum::RxArp{hw.n_hosts, hw.n_queries, hw.n_reply_slots, hw.arp_flags, e.as<fs_arp_host_out>(rxp::kHostsOut),
                           e.as<fs_arp_query_out>(rxp::kQueriesOut), e.as<uint8_t>(rxp::kArpFrames), e.as<fs_digest>(rxp::kArpOut),
                           e.as<uint8_t>(rxp::kArpStatus), e.as<uint8_t>(rxp::kArpCode), e.as<uint32_t>(rxp::kArpOf)};
}

// The ARP call's host form without a batch, as connect_host_empty: nothing is staged but the hosts and the
// queries; the ARP stage alone runs on the compute stream over the context's device arrays (a flagged query
// owes its request, which only the device builds), and its arrays come back.
fs_status arp_host_empty(fs_ctx* ctx, const RxCall& c) {
    RxArpArrays e(c.a.dev);
    e.L = rxp::arp_layout(0, arp_counts(c.a.dev, 0));
    fs_status st = begin_host_call(ctx);
    if (st == FS_SUCCESS) st = ctx->rx_arrays.grow(ctx, e.L.bytes);
    if (st != FS_SUCCESS) return st;
    const hipStream_t ks = ctx->compute_stream;
    ctx->host_dirty = true;
    st = arp_in(ctx, e, ks);
    if (st != FS_SUCCESS) return st;
    RxDevice d{c.b, RxResults{}, ks};
    d.w = arp_device(c.a.dev, e);
    const RxLaunch how{rx_workgroups(ctx), ctx->flow_hash_mask, ctx->flow_steps, ks};
    RxLeft left{};
    st = arp_stage(ctx, c, d, how, left);
    if (st != FS_SUCCESS) {
        drain_host_streams(ctx);
        return st;
    }
    st = arp_back(ctx, e, ks);
    if (st != FS_SUCCESS) return st;
    FS_HIP_DRAIN(ctx, hipStreamSynchronize(ks));
    ctx->host_dirty = false;
    return FS_SUCCESS;
}

// A checked host form: the batch staged through slot 0, the result arrays carved from the context's
// buffer as plan::rx::layout and extra_layout say, the stages, then what they wrote copied back by the same description.
fs_status rx_host(fs_ctx* ctx, const RxCall& c, uint64_t frames_bytes) {
    const RxBatch& b = c.b;
    const RxResults& h = c.r;
    const RxSocks& s = c.s;
    const uint32_t n = b.n;
    const bool sockets = c.kind >= rxp::kDeliver;
    const uint64_t totals_bytes = rxp::totals_bytes(c.kind);
    if (n == 0) {  // nothing for a device to do: the sockets keep their state
        std::memset(h.totals(), 0, totals_bytes);
        for (uint32_t i = 0; sockets && i < s.n_socks; ++i) h.socks_out()[i] = dl::untouched(s.socks[i]);
        for (uint32_t i = 0; c.kind >= rxp::kRecv && i < s.n_socks; ++i)
            h.snd_out()[i] = rv::untouched(s.snd[i].snd_una, s.snd[i].snd_wnd);
        if (c.kind >= rxp::kAccept) {  // no slot is filled, no listener has a candidate
            if (c.l.dev.n_slots) std::memset(c.l.dev.conns, 0, (uint64_t)c.l.dev.n_slots * sizeof(fs_accept_conn));
            if (c.l.dev.n_listeners) std::memset(c.l.dev.listeners_out, 0, (uint64_t)c.l.dev.n_listeners * sizeof(fs_listener_out));
        }
        if (c.kind >= rxp::kClose) {  // no connection has a flow
            for (uint32_t i = 0; i < c.k.dev.n_closers; ++i) c.k.dev.closers_out[i] = cl::untouched_closer(c.k.recs[i]);
            for (uint32_t i = 0; i < s.n_socks; ++i)
                c.k.dev.socks_close[i] = cl::untouched_sock(s.socks[i].rcv_nxt, s.snd[i].snd_una, s.snd[i].snd_wnd, cl::kNone);
        }
        if (c.kind >= rxp::kUdp) {  // no port has a frame: the queues keep their state
            for (uint32_t i = 0; i < c.p.dev.n_ports; ++i) c.p.dev.ports_out[i] = ud::port_out(c.p.recs[i], 0u);
        }
        // no opener has a flow either, yet a flagged one owes its SYN, which only the device builds
        if (c.kind >= rxp::kConnect && c.o.dev.n_openers != 0) {
            const fs_status st = connect_host_empty(ctx, c);
            if (st != FS_SUCCESS) return st;
        }
        // no host has a request and no query a reply, yet a flagged query owes its request
        if (c.kind == rxp::kArp && c.a.dev.n_hosts != 0) return arp_host_empty(ctx, c);
        return FS_SUCCESS;
    }
    RxExtra e(c);  // the own arrays of the accept, the close and the connect call
    const framesum::plan::Scan sc = framesum::plan::scan_batch(b.offsets, b.lengths, n, frames_bytes);
    if (sc.bad < n) return invalid(ctx, c, "frame " + std::to_string(sc.bad) + " ends past frames_bytes");
    // the device payload buffer: payload_cap, or the most payload the batch can hold when that is less
    const uint64_t d_cap = std::min(h.payload_cap, framesum::plan::total_length(b.lengths, n));
    // the rings' span (the kernels address ring bytes at base + ring_off)
    const uint64_t span = s.span.hi - s.span.lo;
    const rxp::Layout L = rxp::layout(c.kind, n, s.n_socks);
    e.L = rxp::extra_layout(rxp::kAccept, c.kind, L.bytes, extra_counts(c));
    // the UDP call's own arrays behind them, and the cells' span (the kernels address cells at base + cells_off)
    const bool udp = c.kind >= rxp::kUdp;
    const framesum::RxUdp& hu = c.p.dev;
    const rxp::UdpLayout UL = rxp::udp_layout(e.L.bytes, udp ? n : 0, udp ? hu.n_ports : 0);
    const uint64_t cspan = c.p.span.hi - c.p.span.lo;
    void* const h_udp[rxp::kUdpArrays] = {hu.ports_out, hu.port_of, hu.cell_of};
    // the ARP call's own arrays behind those
    const bool arp = c.kind == rxp::kArp;
    RxArpArrays ea(c.a.dev);
    ea.L = rxp::arp_layout(UL.bytes, arp ? arp_counts(c.a.dev, n) : rxp::ArpCounts{});
    fs_status st = begin_host_call(ctx);
    if (st == FS_SUCCESS && sockets) st = ctx->dl_rings.grow(ctx, span);
    // (the socket calls begin once more, behind the rings' buffer: a second hipSetDevice that keeps their
    // sequence of HIP calls what profiles/rx_call_refactor/calls.txt compares)
    if (st == FS_SUCCESS && sockets) st = begin_host_call(ctx);
    if (st == FS_SUCCESS) st = ctx->co_payload.grow(ctx, d_cap);
    if (st == FS_SUCCESS) st = ctx->rx_arrays.grow(ctx, ea.L.bytes);
    if (st == FS_SUCCESS && udp) st = ctx->ud_cells.grow(ctx, cspan);
    if (st != FS_SUCCESS) return st;
    Staged sg;
    st = stage_batch(ctx, b.frames, frames_bytes, sc.lo, sc.hi, b.offsets, b.lengths, n, sg);
    if (st != FS_SUCCESS) return st;
    RxDevice d{RxBatch{sg.base, sg.d_off, sg.d_len, n, b.mtu, b.flags}, RxResults{}, sg.ks};
    d.r.payload = ctx->co_payload.p, d.r.payload_cap = d_cap, d.r.out = sg.d_out, d.r.status = sg.d_st;
    d.r.rings = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(ctx->dl_rings.p) - s.span.lo);
    // an array the caller did not pass goes to the launches as a null pointer
    for (uint32_t a = 0; a < rxp::kArrays; ++a) d.r.array[a] = h.array[a] && L.has((rxp::Array)a) ? ctx->rx_arrays.p + L.at[a] : nullptr;
    // the span goes in first, so that the copy back returns the caller's own bytes between the rings
    if (span != 0) FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->dl_rings.p, h.rings + s.span.lo, span, hipMemcpyHostToDevice, sg.ks));
    st = extra_in(ctx, e, sg.ks);
    if (st != FS_SUCCESS) return st;
    d.x = accept_device(c.l.dev, e), d.y = close_device(c.k.dev, e), d.z = connect_device(c.o.dev, e);
    if (udp) {
        const auto at = [&](rxp::UdpArray a) { return h_udp[a] && UL.room[a] ? ctx->rx_arrays.p + UL.at[a] : nullptr; };
        d.u = framesum::RxUdp{hu.n_ports, hu.max_cell, reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(ctx->ud_cells.p) - c.p.span.lo),
                              reinterpret_cast<fs_udp_port_out*>(at(rxp::kPortsOut)), reinterpret_cast<uint32_t*>(at(rxp::kPortOf)),
                              reinterpret_cast<uint32_t*>(at(rxp::kCellOf))};
        // the span goes in first, so that the copy back returns the caller's own bytes around the written cells
        if (cspan != 0)
            FS_HIP_DRAIN(ctx, hipMemcpyAsync(ctx->ud_cells.p, hu.cells + c.p.span.lo, cspan, hipMemcpyHostToDevice, sg.ks));
    }
    if (arp) {
        st = arp_in(ctx, ea, sg.ks);
        if (st != FS_SUCCESS) return st;
        d.w = arp_device(c.a.dev, ea);
    }
    RxLeft left;
    st = rx_run(ctx, c, d, left);
    if (st != FS_SUCCESS) {
        drain_host_streams(ctx);
        return st;
    }
    // the totals and how far the payload got written decide what else comes back
    fs_rx_totals plain{};
    fs_rx_flow_totals by_flow{};
    void* const t = c.kind == rxp::kPlain ? static_cast<void*>(&plain) : &by_flow;
    uint64_t copied = 0;
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(t, d.r.totals(), totals_bytes, hipMemcpyDeviceToHost, sg.ks));
    FS_HIP_DRAIN(ctx, hipMemcpyAsync(&copied, left.copied, 8, hipMemcpyDeviceToHost, sg.ks));
    FS_HIP_DRAIN(ctx, hipStreamSynchronize(sg.ks));
    const rxp::Totals got = c.kind == rxp::kPlain ? rxp::Totals{plain.n_runs, 0, 0}
                                                  : rxp::Totals{by_flow.n_runs, by_flow.n_flows, by_flow.n_accepted};
    if (copied > d_cap || !rxp::consistent(c.kind, n, got)) {
        drain_host_streams(ctx);
        return set_err(ctx, FS_E_HIP, std::string(c.fn) + ": inconsistent totals from the device");
    }
    // one copy back to the caller, skipped when the caller passed no array or nothing is to come back
    const auto back = [&](void* dst, const void* src, uint64_t bytes) {
        return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, sg.ks) : hipSuccess;
    };
    FS_HIP_DRAIN(ctx, back(h.payload, ctx->co_payload.p, copied));
    for (uint32_t a = rxp::kTotals + 1; a < rxp::kArrays; ++a)
        FS_HIP_DRAIN(ctx, back(h.array[a], d.r.array[a], rxp::bytes_back(c.kind, (rxp::Array)a, n, s.n_socks, got)));
    st = extra_back(ctx, e, sg.ks);
    if (st != FS_SUCCESS) return st;
    FS_HIP_DRAIN(ctx, back(s.n_socks ? h.rings + s.span.lo : nullptr, ctx->dl_rings.p, span));
    if (udp) {
        for (uint32_t a = 0; a < rxp::kUdpArrays; ++a)
            FS_HIP_DRAIN(ctx, back(h_udp[a], ctx->rx_arrays.p + UL.at[a], UL.room[a]));
        FS_HIP_DRAIN(ctx, back(hu.n_ports ? hu.cells + c.p.span.lo : nullptr, ctx->ud_cells.p, cspan));
    }
    if (arp) {
        st = arp_back(ctx, ea, sg.ks);
        if (st != FS_SUCCESS) return st;
    }
    FS_HIP_DRAIN(ctx, back(h.out, sg.d_out, (uint64_t)n * sizeof(fs_digest)));
    FS_HIP_DRAIN(ctx, back(h.status, sg.d_st, n));
    st = finish_staged(ctx, sg);
    if (st == FS_SUCCESS) std::memcpy(h.totals(), t, totals_bytes);
    return st;
}

}  // namespace

// ---- The eighteen entry points: fill the record, check, run.

fs_status fs_coalesce_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                            uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                            fs_rx_run* runs, uint32_t* run_of, fs_rx_totals* totals, fs_digest* out, uint8_t* status,
                            void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kPlain, "fs_coalesce_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
}

fs_status fs_coalesce_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                 const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload,
                                 uint64_t payload_cap, fs_rx_run* runs, uint32_t* run_of, fs_rx_totals* totals,
                                 fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kPlain, "fs_coalesce_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}

fs_status fs_coalesce_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                  uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                                  fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                  fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kFlows, "fs_coalesce_flows_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
}

fs_status fs_coalesce_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes,
                                       const uint64_t* offsets, const uint32_t* lengths, uint32_t n, uint32_t mtu,
                                       uint32_t flags, uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs,
                                       fs_rx_flow* flows, uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals,
                                       fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kFlows, "fs_coalesce_flows_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}

fs_status fs_deliver_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                 uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                                 uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                                 uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows,
                                 uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out,
                                 uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kDeliver, "fs_deliver_flows_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
}

fs_status fs_deliver_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                      const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                      const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                      fs_rx_sock_out* socks_out, uint8_t* delivered, uint8_t* payload,
                                      uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                                      uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kDeliver, "fs_deliver_flows_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}

fs_status fs_recv_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                              uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                              uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                              const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, uint8_t* payload,
                              uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                              uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kRecv, "fs_recv_flows_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
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
    RxCall c(rxp::kRecv, "fs_recv_flows_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}

fs_status fs_accept_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                                uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                                const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                                fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                                uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, uint8_t* payload,
                                uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                                uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kAccept, "fs_accept_flows_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
}

fs_status fs_accept_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                     const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                     const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                     fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                     fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                     uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                     uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out,
                                     uint32_t* accept_of, uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status,
                                     uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows,
                                     uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out,
                                     uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kAccept, "fs_accept_flows_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}

fs_status fs_close_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                               uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                               uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                               const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                               uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                               fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                               uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, const fs_cl_sock* closers,
                               uint32_t n_closers, fs_cl_out* closers_out, fs_cl_out* socks_close, uint8_t* ctl_code,
                               uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                               uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kClose, "fs_close_flows_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    c.closing(closers, n_closers, closers_out, socks_close, ctl_code);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
}

fs_status fs_close_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                    const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                    fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                    fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                    uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                    uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out,
                                    uint32_t* accept_of, uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status,
                                    const fs_cl_sock* closers, uint32_t n_closers, fs_cl_out* closers_out,
                                    fs_cl_out* socks_close, uint8_t* ctl_code, uint8_t* payload, uint64_t payload_cap,
                                    fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                    fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kClose, "fs_close_flows_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    c.closing(closers, n_closers, closers_out, socks_close, ctl_code);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}

fs_status fs_connect_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                               uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                               uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                               const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                               uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                               fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                               uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, const fs_cl_sock* closers,
                               uint32_t n_closers, fs_cl_out* closers_out, fs_cl_out* socks_close, uint8_t* ctl_code,
                               const fs_cn_sock* openers, uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out,
                               uint8_t* replies, fs_digest* reply_out, uint8_t* reply_status,
                               uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                               uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kConnect, "fs_connect_flows_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    c.closing(closers, n_closers, closers_out, socks_close, ctl_code);
    c.opening(openers, n_openers, reply_flags, openers_out, replies, reply_out, reply_status);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
}

fs_status fs_connect_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                    const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                    fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                    fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                    uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                    uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out,
                                    uint32_t* accept_of, uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status,
                                    const fs_cl_sock* closers, uint32_t n_closers, fs_cl_out* closers_out,
                                    fs_cl_out* socks_close, uint8_t* ctl_code, const fs_cn_sock* openers,
                                    uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out, uint8_t* replies,
                                    fs_digest* reply_out, uint8_t* reply_status, uint8_t* payload, uint64_t payload_cap,
                                    fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                    fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kConnect, "fs_connect_flows_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    c.closing(closers, n_closers, closers_out, socks_close, ctl_code);
    c.opening(openers, n_openers, reply_flags, openers_out, replies, reply_out, reply_status);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}

fs_status fs_udp_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                               uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                               uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                               const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                               uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                               fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                               uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, const fs_cl_sock* closers,
                               uint32_t n_closers, fs_cl_out* closers_out, fs_cl_out* socks_close, uint8_t* ctl_code,
                               const fs_cn_sock* openers, uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out,
                               uint8_t* replies, fs_digest* reply_out, uint8_t* reply_status,
                               const fs_udp_port* ports, uint32_t n_ports, uint8_t* cells, uint64_t cells_bytes,
                               fs_udp_port_out* ports_out, uint32_t* port_of, uint32_t* cell_of,
                               uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                               uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kUdp, "fs_udp_flows_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    c.closing(closers, n_closers, closers_out, socks_close, ctl_code);
    c.opening(openers, n_openers, reply_flags, openers_out, replies, reply_out, reply_status);
    c.datagrams(ports, n_ports, cells, cells_bytes, ports_out, port_of, cell_of);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
}

fs_status fs_udp_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                    const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                    fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                    fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                    uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                    uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out,
                                    uint32_t* accept_of, uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status,
                                    const fs_cl_sock* closers, uint32_t n_closers, fs_cl_out* closers_out,
                                    fs_cl_out* socks_close, uint8_t* ctl_code, const fs_cn_sock* openers,
                                    uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out, uint8_t* replies,
                                    fs_digest* reply_out, uint8_t* reply_status, const fs_udp_port* ports, uint32_t n_ports,
                                    uint8_t* cells, uint64_t cells_bytes, fs_udp_port_out* ports_out, uint32_t* port_of,
                                    uint32_t* cell_of, uint8_t* payload, uint64_t payload_cap,
                                    fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                    fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kUdp, "fs_udp_flows_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    c.closing(closers, n_closers, closers_out, socks_close, ctl_code);
    c.opening(openers, n_openers, reply_flags, openers_out, replies, reply_out, reply_status);
    c.datagrams(ports, n_ports, cells, cells_bytes, ports_out, port_of, cell_of);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}

fs_status fs_arp_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                               uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                               uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                               const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                               uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                               fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                               uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, const fs_cl_sock* closers,
                               uint32_t n_closers, fs_cl_out* closers_out, fs_cl_out* socks_close, uint8_t* ctl_code,
                               const fs_cn_sock* openers, uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out,
                               uint8_t* replies, fs_digest* reply_out, uint8_t* reply_status,
                               const fs_udp_port* ports, uint32_t n_ports, uint8_t* cells, uint64_t cells_bytes,
                               fs_udp_port_out* ports_out, uint32_t* port_of, uint32_t* cell_of,
                               const fs_arp_host* hosts, uint32_t n_hosts, const fs_arp_query* queries, uint32_t n_queries,
                               uint32_t n_reply_slots, uint32_t arp_flags, fs_arp_host_out* hosts_out,
                               fs_arp_query_out* queries_out, uint8_t* arp_frames, fs_digest* arp_out, uint8_t* arp_status,
                               uint8_t* arp_code, uint32_t* arp_of,
                               uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                               uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kArp, "fs_arp_flows_batch", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    c.closing(closers, n_closers, closers_out, socks_close, ctl_code);
    c.opening(openers, n_openers, reply_flags, openers_out, replies, reply_out, reply_status);
    c.datagrams(ports, n_ports, cells, cells_bytes, ports_out, port_of, cell_of);
    c.neighbours(hosts, n_hosts, queries, n_queries, n_reply_slots, arp_flags, hosts_out, queries_out, arp_frames, arp_out,
                 arp_status, arp_code, arp_of);
    const fs_status st = rx_check(ctx, c, true);
    return st != FS_SUCCESS ? st : rx_device(ctx, c, stream);
}

fs_status fs_arp_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                    const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                    fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                    fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                    uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                    uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out,
                                    uint32_t* accept_of, uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status,
                                    const fs_cl_sock* closers, uint32_t n_closers, fs_cl_out* closers_out,
                                    fs_cl_out* socks_close, uint8_t* ctl_code, const fs_cn_sock* openers,
                                    uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out, uint8_t* replies,
                                    fs_digest* reply_out, uint8_t* reply_status, const fs_udp_port* ports, uint32_t n_ports,
                                    uint8_t* cells, uint64_t cells_bytes, fs_udp_port_out* ports_out, uint32_t* port_of,
                                    uint32_t* cell_of, const fs_arp_host* hosts, uint32_t n_hosts,
                                    const fs_arp_query* queries, uint32_t n_queries, uint32_t n_reply_slots,
                                    uint32_t arp_flags, fs_arp_host_out* hosts_out, fs_arp_query_out* queries_out,
                                    uint8_t* arp_frames, fs_digest* arp_out, uint8_t* arp_status, uint8_t* arp_code,
                                    uint32_t* arp_of, uint8_t* payload, uint64_t payload_cap,
                                    fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                    fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status) {
    if (!ctx) return FS_E_INVALID;
    ctx->err.clear();
    RxCall c(rxp::kArp, "fs_arp_flows_batch_host", RxBatch{frames, offsets, lengths, n, mtu, flags});
    c.coalesce(payload, payload_cap, runs, run_of, totals, out, status);
    c.flows(flows, order);
    c.sockets(socks, n_socks, rings, rings_bytes, socks_out, delivered);
    c.send_side(snd, snd_out, code);
    c.listening(listeners, n_listeners, slots, n_slots, synack_flags, conns, listeners_out, accept_of, synacks, synack_out,
                synack_status);
    c.closing(closers, n_closers, closers_out, socks_close, ctl_code);
    c.opening(openers, n_openers, reply_flags, openers_out, replies, reply_out, reply_status);
    c.datagrams(ports, n_ports, cells, cells_bytes, ports_out, port_of, cell_of);
    c.neighbours(hosts, n_hosts, queries, n_queries, n_reply_slots, arp_flags, hosts_out, queries_out, arp_frames, arp_out,
                 arp_status, arp_code, arp_of);
    const fs_status st = rx_check(ctx, c, false);
    return st != FS_SUCCESS ? st : rx_host(ctx, c, frames_bytes);
}
