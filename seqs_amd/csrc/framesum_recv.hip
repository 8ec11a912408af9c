// The send side of the receive call (fs_recv_flows_batch): behind the launches of the in-order delivery
// (framesum_deliver.hip), whose scratch of the same call these kernels read -- per slot Seq and the
// mark word (`mk`), the ring position (`dwpos`: admitted iff not "none"), per socket its flow's first
// slot (`sock_first`), per flow its socket (`flow_sock`), and the `stop` the delivery's walk has just
// written into socks_out -- fold every listed socket's ACKs and windows (framesum_recv.h).
//
// The launches on the caller's stream, none of which waits on another workgroup or wave of its own
// launch, every loop bounded by a count known at its start:
//   (memset)  `code` to 0.
//   gather    one lane per slot of a matched flow: Ack and the dword at L4 + 12 (flags and window)
//             from the frame at L4 = 14 + 4 IHL, into per-slot scratch, so that the walk's loads are
//             contiguous.
//   walk      one wave per socket: the slots [first, stop) in chunks of 64, the loads of four chunks in
//             flight together. rcv.NXT before each lane is an exclusive wave scan of len + fin over the
//             admitted lanes; snd.UNA before each lane is an exclusive wave scan of functions under
//             composition (framesum_recv.h Fn, run as a minimum over scan_key), with no restart since the
//             receive chain does not depend on the send chain; a chunk that holds an Ack exactly 2^31
//             behind snd_nxt (a wave-uniform ballot) is stepped lane by lane instead. Then every lane
//             decides its code at once; the counts are popcounts of ballots, the window is read from
//             the highest lane with code 1.
#include <hip/hip_runtime.h>

#include <rocprim/warp/warp_scan.hpp>

#include "../../include/framesum_recv.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_flows.h"
#include "framesum_internal.h"
#include "framesum_recv.h"

namespace framesum {

namespace {

using namespace codev;
namespace rv = recv;

struct RvArgs : FlowView {  // (the flow launches' scratch of this call)
    const uint8_t* frames;
    const uint64_t* offsets;
    // the delivery launches' scratch and result of this call
    const uint32_t* flow_sock;
    const uint2* mk;
    const uint32_t* dwpos;
    const uint32_t* sock_first;
    const fs_rx_sock_out* socks_out;
    // the staged block
    const rv::Sock* socks;
    // this call's own scratch
    uint2* aw;  // per slot of a matched flow: Ack, the dword at L4 + 12
    fs_rx_snd_out* snd_out;
    uint8_t* code;
    uint32_t n, n_blocks, n_socks;
};

__global__ void __launch_bounds__(kThreads) recv_gather(const RvArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        if (k >= a.n) continue;
        if (!(a.rec[k].y & kAccepted)) continue;
        if (a.flow_sock[a.flowidx[k]] >= a.n_socks) continue;
        // an accepted TCP frame holds its whole TCP header (the verdict's gates)
        const uint8_t* __restrict__ p = a.frames + a.offsets[slot_frame(a, k)];
        const uint32_t l4 = 14u + 4u * (p[14] & 15u);
        a.aw[k] = make_uint2(__builtin_bswap32(load_at<uint32_t>(p + l4 + 8u)), load_at<uint32_t>(p + l4 + 12u));
    }
}

// What a lane holds of its slot of a chunk. The four loads do not wait for each other.
struct Held {
    uint32_t in, seq, word, ack, dword12, pos, frame;
};
__device__ __forceinline__ Held hold(const RvArgs& a, uint32_t k, uint32_t stop) {
    Held h{0u, 0u, 0u, 0u, 0u, rv::kNone, 0u};
    if (k < stop) {
        const uint2 m = a.mk[k], w = a.aw[k];
        h.pos = a.dwpos[k];
        h.frame = slot_frame(a, k);
        h.in = 1u, h.seq = m.x, h.word = m.y, h.ack = w.x, h.dword12 = w.y;
    }
    return h;
}

// rocPRIM's wave scans: the sum of len + fin, and the minimum of the keys (framesum_recv.h scan_key)
// that stands for the composition of the lanes' functions.
using SumScan = rocprim::warp_scan<uint32_t, 64>;
using KeyScan = rocprim::warp_scan<uint64_t, 64>;
struct ScanStorage {
    SumScan::storage_type sum;
    KeyScan::storage_type key;
};
__device__ __forceinline__ unsigned long long lanes_upto(uint32_t l) { return l >= 63u ? ~0ull : (2ull << l) - 1ull; }

// The walk's state between chunks, the same in all lanes.
struct Walk {
    rv::Snd snd;
    uint32_t nxt;  // rcv.NXT as the delivery's walk has it before the chunk
};

// One chunk of a socket's walk: lane l holds slot base + l in `cur` (the slots of [first, stop) fill the
// lanes from 0 on). Advances `w` and the out record `o`.
__device__ __forceinline__ void walk_chunk(const RvArgs& a, const rv::Sock& sk, uint32_t lane, const Held& cur, Walk& w,
                                           fs_rx_snd_out& o, ScanStorage& storage) {
    const bool in = cur.in != 0u;
    rv::Frame f;
    f.seq = cur.seq, f.ack = cur.ack, f.window = rv::window_of(cur.dword12), f.flags9 = rv::flags9_of(cur.dword12);
    f.len = cur.word & 0xFFFFu;
    f.admitted = in && cur.pos != rv::kNone;
    const uint32_t fin = (f.flags9 & kFin) ? 1u : 0u;
    // rcv.NXT before each lane: it advances by len + fin of the admitted lanes (64 x 65,537 < 2^32)
    const uint32_t adv = f.admitted ? f.len + fin : 0u;
    uint32_t i_adv;
    SumScan().inclusive_scan(adv, i_adv, storage.sum);
    const uint32_t nxt_k = w.nxt + (i_adv - adv);
    // snd.UNA before each lane
    uint32_t my_una;
    const unsigned long long half = __ballot(in && rv::at_half(nxt_k, sk.snd_nxt, f));
    if (half == 0ull) {
        const rv::Fn mine = in ? rv::fn_of(nxt_k, sk.snd_nxt, f) : rv::identity();
        const unsigned long long constants = __ballot(mine.set != 0u);
        const uint64_t key = rv::scan_key(mine, (uint32_t)__popcll(constants & lanes_upto(lane)));
        uint64_t before;  // the minimum over the lanes below this one
        KeyScan().exclusive_scan(key, before, rv::kKeyIdentity, storage.key, rocprim::minimum<uint64_t>());
        const uint32_t d_in = sk.snd_nxt - w.snd.una;
        my_una = sk.snd_nxt - rv::apply(rv::fn_of_key(before), d_in);
        const uint64_t incl = before < key ? before : key;
        const uint64_t all = ((uint64_t)lane_value((uint32_t)(incl >> 32), 63u) << 32) | lane_value((uint32_t)incl, 63u);
        w.snd.una = sk.snd_nxt - rv::apply(rv::fn_of_key(all), d_in);
    } else {
        // the literal rule, one lane after the other (the lanes of the flow come first: at most 64 steps)
        const uint32_t cnt = (uint32_t)__popcll(__ballot(in));
        uint32_t una = w.snd.una;
        my_una = una;
        for (uint32_t l = 0; l < cnt; ++l) {
            if (lane == l) my_una = una;
            rv::Frame g;
            g.seq = lane_value(f.seq, l), g.ack = lane_value(f.ack, l), g.window = 0u, g.flags9 = lane_value(f.flags9, l);
            g.len = lane_value(f.len, l), g.admitted = lane_value(f.admitted ? 1u : 0u, l) != 0u;
            const uint32_t c = rv::code_of(una, lane_value(nxt_k, l), sk.snd_nxt, sk.rcv_wnd, g);
            una = rv::step(rv::Snd{una, 0u}, c, g).una;
        }
        w.snd.una = una;
    }
    const uint32_t code = in ? rv::code_of(my_una, nxt_k, sk.snd_nxt, sk.rcv_wnd, f) : (uint32_t)rv::kNoCode;
    const unsigned long long taken = __ballot(code == rv::kTaken);
    o.n_taken += (uint32_t)__popcll(taken);
    o.n_dup += (uint32_t)__popcll(__ballot(code == rv::kDuplicate));
    o.n_unsent += (uint32_t)__popcll(__ballot(code == rv::kUnsent));
    o.n_rejected += (uint32_t)__popcll(__ballot(code == rv::kRejected || code == rv::kRingFull));
    o.n_keepalive += (uint32_t)__popcll(__ballot(code == rv::kKeepalive));
    if (__ballot(in && rv::owes_ack(code, f)) != 0ull) o.flags |= FS_RECV_ACK_OWED;
    if (__ballot(f.admitted && fin != 0u) != 0ull) o.flags |= FS_RECV_FIN;
    if (taken != 0ull) w.snd.wnd = lane_value(f.window, 63u - (uint32_t)__builtin_clzll(taken));
    w.nxt += lane_value(i_adv, 63u);
    if (in && a.code) a.code[cur.frame] = (uint8_t)code;
}

// Chunks whose loads are in flight together, as the delivery's walk has them.
constexpr uint32_t kAhead = 4;

__global__ void __launch_bounds__(kThreads) recv_walk(const RvArgs a) {
    __shared__ ScanStorage s_scan[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t s = blockIdx.x * kWaves + wave; s < a.n_socks; s += gridDim.x * kWaves) {
        const rv::Sock sk = a.socks[s];
        fs_rx_snd_out o = rv::untouched(sk.snd_una, sk.snd_wnd);
        const uint32_t first = a.sock_first[s];
        if (first < a.n) {
            uint32_t stop = a.socks_out[s].stop;  // (first <= stop <= the accepted slots)
            if (stop > a.n) stop = a.n;
            Walk w{rv::Snd{sk.snd_una, sk.snd_wnd}, sk.rcv_nxt};
            Held cur[kAhead], next[kAhead];
#pragma unroll
            for (uint32_t c = 0; c < kAhead; ++c) cur[c] = hold(a, first + 64u * c + lane, stop);
            // ceil((stop - first) / 256) rounds
            for (uint32_t base = first; base < stop; base += 64u * kAhead) {
#pragma unroll
                for (uint32_t c = 0; c < kAhead; ++c) next[c] = hold(a, base + 64u * (kAhead + c) + lane, stop);
#pragma unroll
                for (uint32_t c = 0; c < kAhead; ++c)
                    if (base + 64u * c < stop) walk_chunk(a, sk, lane, cur[c], w, o, s_scan[wave]);
#pragma unroll
                for (uint32_t c = 0; c < kAhead; ++c) cur[c] = next[c];
            }
            o.snd_una = w.snd.una, o.snd_wnd = w.snd.wnd;
        }
        if (lane == 0) a.snd_out[s] = o;
    }
}

}  // namespace

RecvScratch recv_scratch(uint32_t n) {
    RecvScratch s;
    s.aw = 0;
    s.bytes = 8ull * n;
    return s;
}

hipError_t launch_recv(const RxBatch& b, const RxResults& r, const RxLeft& left, const uint8_t* d_block, uint32_t n_socks,
                       const RxLaunch& how) {
    const uint8_t* const deliver_scratch = left.deliver_scratch;
    const DeliverScratch& ds = left.ds;
    const uint32_t n = b.n;
    const hipStream_t stream = how.stream;
    RvArgs a;
    static_cast<FlowView&>(a) = flow_view(left, n);
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.flow_sock = reinterpret_cast<const uint32_t*>(deliver_scratch + ds.flow_sock);
    a.mk = reinterpret_cast<const uint2*>(deliver_scratch + ds.mk);
    a.dwpos = reinterpret_cast<const uint32_t*>(deliver_scratch + ds.dwpos);
    a.sock_first = reinterpret_cast<const uint32_t*>(deliver_scratch + ds.sock_first);
    a.socks_out = r.socks_out();
    a.socks = reinterpret_cast<const rv::Sock*>(d_block);
    a.aw = reinterpret_cast<uint2*>(left.recv_scratch + left.rs.aw);
    a.snd_out = r.snd_out();
    a.code = r.code();
    a.n = n;
    const ScanGrid g = scan_grid(n, how);
    a.n_blocks = g.blocks;
    a.n_socks = n_socks;
    const uint32_t walk_blocks = (n_socks + kWaves - 1u) / kWaves;
    if (n != 0) hipLaunchKernelGGL(recv_gather, dim3(g.scan), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(recv_walk, dim3(g.capped(walk_blocks)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace framesum
