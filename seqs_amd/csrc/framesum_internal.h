// Internal declarations shared by the framesum HIP kernels and the C-ABI host code: the CRC tables'
// layout and the launch entry points. The kernel-choice policy and the constants of the report
// protocol between the kernels and the host are in framesum_choice.h (no HIP there).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "../../include/framesum.h"
#include "../../include/framesum_deliver.h"
#include "../../include/framesum_recv.h"
#include "../../include/framesum_accept.h"
#include "../../include/framesum_close.h"
#include "../../include/framesum_connect.h"
#include "../../include/framesum_udp.h"
#include "../../include/framesum_arp.h"
#include "framesum_choice.h"
#include "framesum_plan.h"

namespace framesum {

// CRC-32 "zero-shift" operator tables, built on the host once per context
// (framesum_tables.cpp) in the kernel's LDS layout.
// Z_k[b][v] = register value after feeding k zero bytes to a reflected
// CRC-32 register holding (v << 8b)  -- i.e. multiplication by x^(8k) mod P.
// Each workgroup builds region A itself from `z64_basis` (VALU + ds_write, no memory
// traffic ahead of the first rows) and copies the plain tables by LDS-DMA behind its
// first rows; they are only needed by the per-frame combine.
struct FsTables {
    // Region A (64 KB): 256 entry rows x 64 dword slots. Slot 8*b + c (c = 0..7) holds
    // Z_64[b][e] (one 64-byte frame-row of stream stride); the 8 copies make the kernel's
    // lookups LDS-bank-conflict-free (the 256-B entry stride lets one v_perm_b32 form the
    // address). Slots 32..63 are unused (the captured header slots do not overlap them).
    uint32_t region_a[256][64];
    uint32_t z32[4][256];      // Z_32 : lane-tree level 1 (lanes l, l+2)
    uint32_t z16[4][256];      // Z_16 : lane-tree level 2 (lanes l, l+1)
    uint32_t zfin[4][4][256];  // Z_4, Z_3, Z_2, Z_1 : final step Z_(4-t) (t = bytes of dword rounding); Z_4 also
                               // serves the intra-lane combine
    uint32_t z48[4][256];      // Z_48 : lane 0 of the flattened lane tree
    uint32_t z12[4][256];      // Z_12 : stream 0 of the flattened intra-lane combine
    uint32_t z8[4][256];       // Z_8  : stream 1
    uint32_t z768[4][256];     // Z_768: one full piece (mode B Horner over a frame's pieces)
    // --- not part of the LDS image ---
    uint32_t z64_basis[4][8];  // Z_64[b][1 << j]: region A's entries are XORs of these
    // T[b][1 << j] of the 40 plain [4][256] tables above, in LDS-image order (piece p = 4 t + b is the
    // 1-KB piece at LDS byte 1024 p): the kernels build them in place by VALU, as region A
    uint32_t plain_basis[40][8];
};
constexpr uint32_t kTablesLdsBytes = 65536 + 4096 * 10;  // the LDS image: everything before z64_basis
static_assert(offsetof(FsTables, z64_basis) == kTablesLdsBytes, "FsTables layout");
static_assert(offsetof(FsTables, z32) == 65536 && offsetof(FsTables, plain_basis) == kTablesLdsBytes + 128,
              "FsTables layout: the plain tables are 40 1-KB pieces after region A");

void build_tables(FsTables* t);

// Launch one batch: choose() (framesum_choice.h) picks the kernel from the context's choice `state`
// and its host-mapped report block (`report_host` / `report_dev`: the same 64 B as the host and the
// device address them, nullable), the grid is sized for `num_cus` workgroups, and the kernel is
// enqueued on `stream`. The choice never changes a result, only the speed. `force`: a kKernel* value
// (fs_ctx_set_kernel; tests run every case through each) or one of the host-staged path's kForce*
// values.
// `op`: the RX digest; the TX fill (`wframes` = the same frames, writable; `tx` = FS_FILL_* flags:
// checksums written into the frames and/or the FCS appended after them); or the RX digest of
// wire frames whose lengths include a trailing FCS.
enum class FsOp { kDigest, kFill, kFcs };
hipError_t launch_digest(const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                         uint32_t mtu, const FsTables* tables, void* out, uint8_t* status, hipStream_t stream,
                         int num_cus, ChoiceState& state, const volatile uint32_t* report_host, uint32_t* report_dev,
                         int force = 0, FsOp op = FsOp::kDigest, uint8_t* wframes = nullptr, uint32_t tx = 0);

// Restore global frame order from nshards gathered round-robin slabs (framesum_plan.h layout):
// out[i] = slab[i % nshards].digest[i / nshards], status likewise (nullable), for global frames
// [i0, min(i1, n)) of the n-frame batch. framesum_shard.hip.
hipError_t launch_deinterleave(const uint8_t* gathered, uint32_t nshards, uint64_t n, void* out, uint8_t* status,
                               hipStream_t stream, uint64_t i0 = 0, uint64_t i1 = ~0ull);

// ---- TX frame build (framesum_segment.hip; the device code it shares with the ring send:
// framesum_tx_dev.h). The kernels' CRC zero-shift tables Z_1, Z_2, Z_4, ...
// Z_32768 (tables 0..15) and Z_12 (table 16) as their one-bit basis, basis[t][b][j] = Z_k[b][1 << j]:
// every workgroup expands them into LDS.
constexpr uint32_t kSegTableCount = 17, kSegTableZ12 = 16;
struct SegTables {
    uint32_t basis[kSegTableCount][4][8];
};
void build_segment_tables(SegTables* t);

namespace segment {
struct Block;
}
// One launch that builds the n_frames frames of a staged batch: `d_block` is the device copy of the
// block segment::stage() filled (framesum_segment.h), `b` its layout. `workgroups` caps the grid.
hipError_t launch_segment(const uint8_t* d_block, const segment::Block& b, uint32_t n_sends, uint32_t n_frames,
                          const uint8_t* payload, uint8_t* frames, uint64_t* offsets, uint32_t* lengths, void* out,
                          uint8_t* status, uint32_t mtu, uint32_t flags, uint32_t align, const SegTables* tables,
                          int workgroups, hipStream_t stream);

// ---- Ring send (framesum_send.hip). One launch that builds the n_frames frames of a staged batch of
// sockets from their TX rings in `rings`: `d_block` is the device copy of the block send::stage()
// filled (framesum_send.h: n_recs records, one per socket that makes a frame), `b` its layout. The
// tables are the TX frame build's. `workgroups` caps the grid.
hipError_t launch_send_rings(const uint8_t* d_block, const segment::Block& b, uint32_t n_recs, uint32_t n_frames,
                             const uint8_t* rings, uint8_t* frames, uint64_t* offsets, uint32_t* lengths, void* out,
                             uint8_t* status, uint32_t mtu, uint32_t flags, uint32_t align, const SegTables* tables,
                             int workgroups, hipStream_t stream);

// ---- Resident ring send (framesum_send_resident.hip; its arithmetic: framesum_send_resident.h). The four
// launches of fs_send_rings_resident: the three plan kernels over `c`'s device socket table, which leave the
// head and send::stage's block in `scratch` (laid out as `sl`), and the frame kernel behind them, whose grid
// is sized from c.frames_cap. `plan_workgroups` and `tx_workgroups` cap the grids.
namespace resident {
struct Call;
struct Scratch;
}  // namespace resident
hipError_t launch_send_resident(resident::Call c, uint8_t* scratch, const resident::Scratch& sl, const uint8_t* rings,
                                uint8_t* frames, uint64_t* offsets, uint32_t* lengths, void* out, uint8_t* status,
                                uint32_t mtu, const SegTables* tables, int plan_workgroups, int tx_workgroups,
                                hipStream_t stream);

// ---- The RX calls (framesum_coalesce.hip, framesum_flows.hip, framesum_deliver.hip, framesum_recv.hip,
// framesum_accept.hip, framesum_close.hip, framesum_connect.hip, framesum_udp.hip, framesum_arp.hip). A call is a row of stages on one stream --
// the digest launch and the plain or the flow-aware gather, then the delivery, then the receive call's fold,
// then the accept call's passive open, then the close call's control walks, then the connect call's active
// open, then the UDP call's delivery into port queues, then the ARP call's replies and resolutions -- each behind the one before it and reading what it left. The launches take the call as a few records.

// The batch as the launches read it.
struct RxBatch {
    const uint8_t* frames;
    const uint64_t* offsets;
    const uint32_t* lengths;
    uint32_t n, mtu, flags;
};
// Where the results go on the device: the caller's pointers in the device forms, the context's device
// arrays in the host forms. `array` holds the arrays framesum_plan.h describes (plan::rx::Array), null
// where the call has none or the caller passed none (the kernels skip those stores); the accessors
// give them their types. `totals` is an fs_rx_totals in the plain call, an fs_rx_flow_totals in the others.
struct RxResults {
    uint8_t* payload;
    uint64_t payload_cap;
    fs_digest* out;
    uint8_t* status;
    uint8_t* rings;
    void* array[plan::rx::kArrays];
    template <class T>
    T* as(plan::rx::Array a) const { return static_cast<T*>(array[a]); }
    void* totals() const { return array[plan::rx::kTotals]; }
    fs_rx_run* runs() const { return as<fs_rx_run>(plan::rx::kRuns); }
    fs_rx_flow* flows() const { return as<fs_rx_flow>(plan::rx::kFlowRecs); }
    uint32_t* order() const { return as<uint32_t>(plan::rx::kOrder); }
    uint32_t* run_of() const { return as<uint32_t>(plan::rx::kRunOf); }
    uint8_t* delivered() const { return as<uint8_t>(plan::rx::kDelivered); }
    fs_rx_sock_out* socks_out() const { return as<fs_rx_sock_out>(plan::rx::kSocksOut); }
    fs_rx_snd_out* snd_out() const { return as<fs_rx_snd_out>(plan::rx::kSndOut); }
    uint8_t* code() const { return as<uint8_t>(plan::rx::kCode); }
};
// How a call's own launches (not the digest's) go: `max_workgroups` caps every grid; `hash_mask` is ANDed
// with a key's hash (all ones in the product); `steps`: which of the flow launches' three groups to
// enqueue, all of them in every call of the ABI (the test library times the sort alone on the keys an
// earlier call has left).
constexpr uint32_t kFlowStepOrder = 1, kFlowStepSort = 2, kFlowStepGather = 4, kFlowStepsAll = 7;
struct RxLaunch {
    int max_workgroups;
    uint32_t hash_mask, steps;
    hipStream_t stream;
};

// The scratch layouts. CoScratch: the plain gather's, 8-byte aligned; `copied` is the 64-bit count of
// leading payload bytes the copy writes (the whole of it unless payload_cap cuts it short).
// FlowScratch: the flow launches', 256-byte aligned (flows_scratch asks the sort for its temporary
// storage's size, so callers compute it once per call). DeliverScratch and RecvScratch: 8-byte aligned.
struct CoScratch {
    uint64_t rec, payoff, partial, prefix, copied, runidx, hidx, bytes;
};
struct FlowScratch {
    uint64_t keys, sk_in, sorted, rec, payoff, partial, prefix, copied, table, rep, slot_of, runidx, hidx, flowidx, fhidx,
        sort_temp, sort_bytes, bytes;
};
struct DeliverScratch {
    uint64_t mk, dwpos, sock_first, flow_sock, bytes;
};
struct RecvScratch {
    uint64_t aw, bytes;
};
// AcceptScratch: 256-byte aligned like FlowScratch (accept_scratch asks the sort for its temporary
// storage's size too); 20 bytes per frame and 88 per slot beside it.
struct AcceptScratch {
    uint64_t rank_in, rank_sorted, synrec, cand_frame, sort_temp, sort_bytes, bytes;
};
// OwnerScratch: what the match and the gather of the close and of the connect call fill (framesum_match_dev.h:
// an "owner" is a closer or an opener), 16-byte aligned; 20 bytes per frame and 4 per owner. The close call's
// scratch is this; the connect call's has its reply records (`reprec`, 88 per opener, 8-byte aligned) behind it.
struct OwnerScratch {
    uint64_t sq, flow_owner, owner_first, bytes;
};
struct ConnectScratch : OwnerScratch {
    uint64_t reprec;
};
// UdpScratch: 256-byte aligned like AcceptScratch (udp_scratch asks the sort for its temporary storage's
// size too); 20 bytes per frame beside it.
struct UdpScratch {
    uint64_t rank_in, rank_sorted, cell_at, sort_temp, sort_bytes, bytes;
};
CoScratch coalesce_scratch(uint32_t n);
FlowScratch flows_scratch(uint32_t n);
DeliverScratch deliver_scratch(uint32_t n, uint32_t n_socks);
RecvScratch recv_scratch(uint32_t n);
AcceptScratch accept_scratch(uint32_t n, uint32_t n_listeners, uint32_t n_slots);
OwnerScratch owner_scratch(uint32_t n, uint32_t n_owners);
ConnectScratch connect_scratch(uint32_t n, uint32_t n_openers);
UdpScratch udp_scratch(uint32_t n, uint32_t n_ports);
// ArpScratch: 256-byte aligned like UdpScratch (arp_scratch asks the sort for its temporary storage's size
// when a host is listed); 16 bytes per frame, 8 per reply slot and 8 per query beside it.
struct ArpScratch {
    uint64_t rank_in, rank_sorted, slot_frame, slot_host, win, n_rep, sort_temp, sort_bytes, bytes;
};
ArpScratch arp_scratch(uint32_t n, uint32_t n_hosts, uint32_t n_queries, uint32_t n_reply_slots);
// The UDP call's rank-by-sort (framesum_udp.hip): 64-bit keys over their low `bits` bits; with a null
// `temp` it only reports the temporary storage it needs.
hipError_t rank_sort_keys(void* temp, size_t& temp_bytes, uint64_t* in, uint64_t* out, uint32_t n, uint32_t bits,
                          hipStream_t stream);

// What the accept call has beside a receive call's batch and results: the counts of its staged lists and
// where its own results go on the device (the caller's pointers in the device form, the context's device
// arrays in the host form; accept_of, synack_out and synack_status are nullable).
struct RxAccept {
    uint32_t n_socks, n_listeners, n_slots, synack_flags;
    fs_accept_conn* conns;
    fs_listener_out* listeners_out;
    uint32_t* accept_of;
    uint8_t* synacks;
    fs_digest* synack_out;
    uint8_t* synack_status;
};

// What the close call has beside an accept call's: the counts of its lists and where its own results go
// on the device (ctl_code is nullable).
struct RxClose {
    uint32_t n_socks, n_closers;
    fs_cl_out* closers_out;
    fs_cl_out* socks_close;
    uint8_t* ctl_code;
};

// What the connect call has beside a close call's: the count of its list and where its own results go on
// the device (reply_out and reply_status are nullable); ctl_code is the close call's array.
struct RxConnect {
    uint32_t n_openers, reply_flags;
    fs_cn_out* openers_out;
    uint8_t* replies;
    fs_digest* reply_out;
    uint8_t* reply_status;
    uint8_t* ctl_code;
};

// What the UDP call has beside a connect call's: the count of its list and where its own results go on
// the device (port_of and cell_of are nullable). `cells`: the base the ports' cells_off count from.
struct RxUdp {
    uint32_t n_ports, max_cell;  // (max_cell: the list's largest cell_size, which decides the copy's lanes)
    uint8_t* cells;
    fs_udp_port_out* ports_out;
    uint32_t* port_of;
    uint32_t* cell_of;
};

// What the ARP call has beside a UDP call's: the counts of its lists and where its own results go on the
// device (arp_out, arp_status, arp_code and arp_of are nullable).
struct RxArp {
    uint32_t n_hosts, n_queries, n_reply_slots, arp_flags;
    fs_arp_host_out* hosts_out;
    fs_arp_query_out* queries_out;
    uint8_t* arp_frames;
    fs_digest* arp_out;
    uint8_t* arp_status;
    uint8_t* arp_code;
    uint32_t* arp_of;
};

// What the stages of one call leave on the device for the stages behind them: each stage's scratch, laid
// out as its layout says (all zero for a stage that has not run: an empty batch has no flow stage), and
// where the gather's count of written payload bytes lies.
struct RxLeft {
    const uint8_t* copied;
    uint8_t* flow_scratch;
    FlowScratch fs;
    uint8_t* deliver_scratch;
    DeliverScratch ds;
    uint8_t* recv_scratch;
    RecvScratch rs;
    uint8_t* accept_scratch;
    AcceptScratch acs;
    uint8_t* close_scratch;
    OwnerScratch cs;
    uint8_t* connect_scratch;
    ConnectScratch cns;
    uint8_t* udp_scratch;
    UdpScratch us;
    uint8_t* arp_scratch;
    ArpScratch ars;
};

// The launches that follow a batch's digest launch on the stream (fs_coalesce_batch in
// include/framesum.h): classify, the scan's three steps and the copy. `r.status`: the batch's verdicts,
// as that digest launch writes them. `scratch`: coalesce_scratch(n).bytes of device memory.
hipError_t launch_coalesce(const RxBatch& b, const RxResults& r, uint8_t* scratch, const RxLaunch& how);
// ... (fs_coalesce_flows_batch): the delivery order (keys, flow table, sort keys), the sort, and the
// scans and the copy over delivery slots, in `left.flow_scratch` laid out as `left.fs`.
hipError_t launch_coalesce_flows(const RxBatch& b, const RxResults& r, const RxLeft& left, const RxLaunch& how);
// The launches that follow a batch's flow launches (fs_deliver_flows_batch in
// include/framesum_deliver.h) and read what those left. `d_block`: the device copy of the staged block
// (framesum_deliver.h block_of: the socket records, then the socket table). With n of 0 only the
// sockets' out records are written.
hipError_t launch_deliver(const RxBatch& b, const RxResults& r, const RxLeft& left, const uint8_t* d_block, uint32_t n_socks,
                          const RxLaunch& how);
// The launches that follow a batch's delivery launches (fs_recv_flows_batch in include/framesum_recv.h)
// and read what the flow and the delivery launches left, and `r.socks_out()`. `d_block`: the device copy
// of the staged block (framesum_recv.h stage: one Sock per socket). `r.code()` is zeroed by the caller.
// With n of 0 only the sockets' out records are written.
hipError_t launch_recv(const RxBatch& b, const RxResults& r, const RxLeft& left, const uint8_t* d_block, uint32_t n_socks,
                       const RxLaunch& how);
// The launches that follow a non-empty batch's receive launches (fs_accept_flows_batch in
// include/framesum_accept.h) and read what the flow and, with sockets listed, the delivery launches left.
// `d_block`: the device copy of the staged block (framesum_accept.h block_of: the listeners, their table,
// the slots; at least one listener). `tables`: the TX frame build's, and `tx_workgroups` the cap of the
// SYN-ACK kernel's grid as that build has it. x.conns, x.listeners_out and x.accept_of are set to their
// "nothing" values by the caller.
hipError_t launch_accept(const RxBatch& b, const RxAccept& x, const RxLeft& left, const uint8_t* d_block,
                         const SegTables* tables, int tx_workgroups, const RxLaunch& how);

// The launches that follow a batch's accept launches (fs_close_flows_batch in include/framesum_close.h)
// and read what the flow launches and, with sockets listed, the delivery and the receive launches left,
// `r.socks_out()` and `r.snd_out()`. `d_block`: the device copy of the staged block (framesum_close.h
// block_of: the closers, their table, the listed sockets' fixed values); at least one closer or one
// socket. y.ctl_code is zeroed by the caller. With n of 0 only the out records are written.
hipError_t launch_close(const RxBatch& b, const RxResults& r, const RxClose& y, const RxLeft& left, const uint8_t* d_block,
                        const RxLaunch& how);
// The gather of the close and of the connect call (framesum_close.hip), one launch behind the call's match: per
// slot of a flow whose owner is below n_owners, Seq, Ack, the dword at L4 + 12 and the payload length into
// `scratch` laid out as `s`. Enqueues only: the caller asks for the last error behind its launches.
void launch_flow_gather_sq(const RxBatch& b, const RxLeft& left, uint8_t* scratch, const OwnerScratch& s, uint32_t n_owners,
                           const RxLaunch& how);

// The launches that follow a batch's close launches (fs_connect_flows_batch in include/framesum_connect.h)
// and read what the flow launches left. `d_block`: the device copy of the staged block (framesum_connect.h
// block_of: the openers, then their table); at least one opener. `tables` and `tx_workgroups`: as
// launch_accept's, for the reply kernel. With n of 0 only the out records and the flagged SYNs are written.
hipError_t launch_connect(const RxBatch& b, const RxResults& r, const RxConnect& z, const RxLeft& left, const uint8_t* d_block,
                          const SegTables* tables, int tx_workgroups, const RxLaunch& how);

// The launches that follow a batch's connect launches (fs_udp_flows_batch in include/framesum_udp.h) and
// read the verdicts and, when every step of the flow launches ran, the key records those left. `d_block`:
// the device copy of the staged block (framesum_udp.h block_of: the ports, then their table); at least one
// port. With n of 0 only the out records are written.
hipError_t launch_udp(const RxBatch& b, const RxResults& r, const RxUdp& u, const RxLeft& left, const uint8_t* d_block,
                      const RxLaunch& how);

// The launches that follow a batch's UDP launches (fs_arp_flows_batch in include/framesum_arp.h) and read
// the verdicts. `d_block`: the device copy of the staged block (framesum_arp.h block_of), null with no host
// listed: then one launch writes x.arp_code and x.arp_of and nothing else. `tables` and `tx_workgroups`: as
// launch_accept's, for the frame kernel. With n of 0 only the out records and the flagged requests are written.
hipError_t launch_arp(const RxBatch& b, const RxResults& r, const RxArp& x, const RxLeft& left, const uint8_t* d_block,
                      const SegTables* tables, int tx_workgroups, const RxLaunch& how);

}  // namespace framesum
