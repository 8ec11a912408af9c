// Internal to the host side of the C ABI (framesum_api.cpp: context lifecycle, digest and fill calls;
// framesum_api_tx.cpp: the TX frame build; framesum_api_rx.cpp: the nine RX call kinds -- the plain and
// the flow-aware coalesce, the delivery into socket rings, the receive call, the accept call, the close call,
// the connect call, the UDP call and the ARP call): the context, the error
// helpers and macros, the grow-only device buffer, the staging blocks and the launch behind one, and the
// staging helpers of the host-staged calls that stage one batch through slot 0. Defined in
// framesum_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>

#include "../../include/framesum.h"
#include "framesum_internal.h"
#include "framesum_plan.h"

// Host-staged path: the batch is cut into chunks of about kChunkBytes of frame bytes,
// staged through kHostSlots device buffers. The whole batch's descriptors go first, in one
// H2D copy; the chunks' frame bytes then alternate between two copy streams (two DMA queues
// keep the PCIe link busier than one: no gap between one chunk's copy and the next); kernels
// and the small D2H copies run on a compute stream. Events order each chunk's kernel after
// its copy (`copied`) and the reuse of a slot by chunk c + kHostSlots after chunk c's kernel
// (`consumed`), so chunk c+1's H2D overlaps chunk c's kernel and D2H.
constexpr int kHostSlots = 3;
constexpr uint64_t kChunkBytes = 16ull << 20;
constexpr uint32_t kChunkFrames = 1u << 20;
// Frames per call: tile and frame indices are 32-bit in the kernel (n + 15 must not wrap).
constexpr uint32_t kMaxFrames = 1u << 31;

// A grow-only device buffer, freed with the context.
struct DevBuf {
    uint8_t* p = nullptr;
    uint64_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // At least `bytes` bytes (and 256 more: the kernels read past frame ends), the contents lost when
    // it grows; `what` names the buffer in the FS_E_NOMEM message.
    fs_status grow(fs_ctx* ctx, uint64_t bytes, const char* what = "hipMalloc of a staging buffer");
    void release();
    template <class T>
    T* as(uint64_t at = 0) const { return reinterpret_cast<T*>(p + at); }
};

struct HostSlot {
    hipEvent_t copied = nullptr, consumed = nullptr, landed = nullptr;  // landed: the chunk's results are in the mirror
    bool used = false;
    DevBuf frames, offsets, lengths, out, status;
};

// fs_segment_batch stages each call's sends in a block of its own: pinned host memory the call
// fills, a device copy the kernel reads, and an event recorded behind the kernel. A block is
// refilled only once its event has completed, so calls need no synchronization between them.
constexpr int kSegStages = 32;
struct SegStage {
    uint8_t* h = nullptr;
    uint8_t* d = nullptr;
    uint64_t cap = 0;
    hipEvent_t done = nullptr;
    bool used = false;
};

struct fs_ctx {
    int device = 0;
    int num_cus = 0;
    framesum::FsTables* d_tables = nullptr;
    // fault injection for the host-staged pipeline's tests, settable only through the test
    // library's fs_test_set_fault (-DFS_TEST_HOOKS): fs_digest_batch_host fails with FS_E_NOMEM at
    // chunk k, after the earlier chunks' work and chunk k's copy are queued. -1 in the product.
    long fault_chunk = -1;
    // the path the latest fs_digest_batch_host took (fs_test_last_host_path): 1 staged in one
    // chunk, 2 read in place, 3 chunked
    int last_host_path = 0;
    // the host-mapped block the kernels post their reports to (framesum_choice.h), and what the
    // context remembers of them between launches
    volatile uint32_t* h_report = nullptr;
    uint32_t* d_report = nullptr;
    framesum::ChoiceState choice;
    int force_kernel = 0;  // fs_ctx_set_kernel
    int workgroups = 0;    // fs_ctx_set_workgroups (0: one per CU)
    HostSlot slot[kHostSlots];
    hipStream_t copy_stream = nullptr, compute_stream = nullptr;
    hipStream_t copy_stream2 = nullptr;  // the odd chunks' frame copies
    hipEvent_t desc_copied = nullptr;    // the batch's descriptors are on the device
    hipEvent_t host_done = nullptr;      // a host-staged call's last device work (polled, host_wait)
    // a host-staged call left work in flight (it failed half-way): the next one drains the
    // context's streams first (begin_host_call); a call that returns FS_SUCCESS leaves none
    bool host_dirty = false;
    DevBuf desc;  // the batch's offsets (8 n) then lengths (4 n)
    // pinned host mirrors of the descriptors and results, so every per-chunk copy is
    // asynchronous even when the caller's arrays are pageable (Go slices, numpy)
    uint8_t* h_pin = nullptr;
    uint8_t* d_pin = nullptr;  // h_pin as the device addresses it (mapped): kernels write results there
    uint64_t cap_pin_n = 0;
    // TX frame build: the kernel's table basis (built on the first call), the staging blocks, and
    // the device buffers of fs_segment_batch_host (payload, frames, the four result arrays)
    framesum::SegTables* d_seg_tables = nullptr;
    SegStage seg_stage[kSegStages];
    int seg_next = 0;  // the block to wait for when all are busy
    DevBuf seg_payload, seg_frames, seg_arrays;
    // The RX calls. The plain coalesce: the kernels' scratch, and out / status when the caller passes
    // none. The four host forms share the device payload and one buffer of result arrays, laid out per
    // call by plan::rx::layout (framesum_plan.h).
    DevBuf co_scratch, co_results, co_payload, rx_arrays;
    // flow-aware RX coalesce: the kernels' scratch. The hash mask and the steps are all ones / all
    // steps unless the test library's setters change them.
    DevBuf fl_scratch;
    uint32_t flow_hash_mask = 0xFFFFFFFFu;
    uint32_t flow_steps = framesum::kFlowStepsAll;
    // in-order TCP delivery: the kernels' scratch, and the rings' span of the host forms. Its socket
    // block is staged through seg_stage, like the sends of fs_segment_batch.
    DevBuf dl_scratch, dl_rings;
    // the receive call: the kernels' scratch; the call's block is staged through seg_stage like the
    // delivery's.
    DevBuf rv_scratch;
    // the accept call: the kernels' scratch; the listeners, their table and the slots are staged through
    // seg_stage like the delivery's block, and the SYN-ACK kernel reads d_seg_tables.
    DevBuf ac_scratch;
    // the close call: the kernels' scratch; the closers, their table and the sockets' fixed values are
    // staged through seg_stage like the delivery's block.
    DevBuf cl_scratch;
    // the connect call: the kernels' scratch; the openers and their table are staged through seg_stage
    // like the delivery's block, and the reply kernel reads d_seg_tables.
    DevBuf cn_scratch;
    // the UDP call: the kernels' scratch, and the cells' span of the host form; the ports and their table
    // are staged through seg_stage like the delivery's block.
    DevBuf ud_scratch, ud_cells;
    // the ARP call: the kernels' scratch; the hosts, the queries and their tables are staged through
    // seg_stage like the delivery's block, and the frame kernel reads d_seg_tables.
    DevBuf ar_scratch;
    // the resident ring send: the plan kernels' sums, the head and the block they stage for the frame kernel
    // (framesum_send_resident.h scratch_of)
    DevBuf sr_scratch;
    std::string err;
};

namespace framesum {
namespace host {

// The message fs_last_error gives for `ctx`, or for the calling thread (g_create_err) when ctx is null
// (fs_ctx_create, fs_segment_layout); returns `code`.
extern thread_local std::string g_create_err;
fs_status set_err(fs_ctx* ctx, fs_status code, const std::string& msg);
fs_status hip_err(fs_ctx* ctx, hipError_t e, const char* what);

#define FS_HIP(ctx, call)                                                      \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) return framesum::host::hip_err(ctx, e_, #call);  \
    } while (0)

// Every host-staged entry point starts here, behind hipSetDevice of the context's device: the pinned
// mirrors and the staging slots are free only once the context's compute stream AND both copy streams
// are idle (a host-staged call that failed half-way may have left odd-chunk copies in flight on
// copy_stream2 that would otherwise write a slot while the next call stages into it). A call that
// succeeded left nothing in flight (its results were waited for), so the three synchronizes (~3 us each
// when idle) run only after a failed call.
fs_status begin_host_call(fs_ctx* ctx);

// A host-staged call that fails after it has enqueued work drains the context's streams before it
// returns (best effort), so that nothing of it still reads the caller's buffers or writes the
// caller's result arrays (the kernel writes them in place when they are pinned) after the error.
void drain_host_streams(fs_ctx* ctx);
#define FS_HIP_DRAIN(ctx, call)                          \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) {                          \
            framesum::host::drain_host_streams(ctx);     \
            return framesum::host::hip_err(ctx, e_, #call); \
        }                                                \
    } while (0)

// A staging block (fs_ctx::seg_stage) of at least `bytes` bytes whose previous kernel has ended; the
// caller fills `h`, copies it to `d`, sets `used` and records `done` behind its last reader
// (staged_launch below). framesum_api_tx.cpp.
fs_status stage_block(fs_ctx* ctx, uint64_t bytes, SegStage** out);
// One staged block and the launches that read it (the TX frame builds, the delivery, the receive call):
// a block of `bytes` bytes that `fill(h_block)` fills, its copy to the device on `stream`, the launches
// `launch(d_block)` starts behind it on the device copy, and the block's event behind them, recorded
// even when the launch failed (the block may be read by what did get queued). `launch_what` names a
// failed launch in the error text, which comes before the event's. Nothing is allocated.
template <class Fill, class Launch>
fs_status staged_launch(fs_ctx* ctx, uint64_t bytes, hipStream_t stream, const char* launch_what, const Fill& fill,
                        const Launch& launch) {
    SegStage* sg = nullptr;
    const fs_status st = stage_block(ctx, bytes, &sg);
    if (st != FS_SUCCESS) return st;
    fill(sg->h);
    FS_HIP(ctx, hipMemcpyAsync(sg->d, sg->h, bytes, hipMemcpyHostToDevice, stream));
    sg->used = true;  // (from here on the block may be read by queued work)
    const hipError_t le = launch(static_cast<const uint8_t*>(sg->d));
    const hipError_t re = hipEventRecord(sg->done, stream);
    if (le != hipSuccess) return hip_err(ctx, le, launch_what);
    if (re != hipSuccess) return hip_err(ctx, re, "hipEventRecord(sg->done, stream)");
    return FS_SUCCESS;
}
// fs_ctx::d_seg_tables, built and uploaded on the first call of a frame-building kernel
// (fs_segment_batch, fs_send_rings_batch). framesum_api_tx.cpp.
fs_status seg_tables(fs_ctx* ctx);

// Where a frame-building call (fs_segment_batch, fs_send_rings_batch and their host forms) reads and
// writes on the device: `src` is what the records' byte offsets count in (the payload, the rings), the
// four result arrays are nullable.
struct TxDevice {
    const uint8_t* src;
    uint8_t* frames;
    uint64_t* offsets;
    uint32_t* lengths;
    fs_digest* out;
    uint8_t* status;
    hipStream_t stream;
};
// What such a call enqueues on `stream` for a checked batch: the tables, then staged_launch of a block
// of `block_bytes` bytes that `fill` fills and of the one kernel that `launch` starts on the device copy
// with at most `workgroups` workgroups. `launch_what` names a failed launch in the error text. (Pass
// the callables by std::ref: nothing is allocated then.) framesum_api_tx.cpp.
fs_status tx_enqueue(fs_ctx* ctx, uint64_t block_bytes, const std::function<void(uint8_t* h_block)>& fill,
                     const std::function<hipError_t(const uint8_t* d_block, int workgroups)>& launch,
                     const char* launch_what, hipStream_t stream);
// The device round trip of such a call's host form, on the compute stream: bytes [lo, hi) of `src`
// go to the device, and the caller's frames span when the slots leave `gaps` (the kernel writes frame
// and FCS bytes only); `enqueue` gets the device buffers, with `src` rebased so that the records'
// offsets hold; the frames and the result arrays the caller passed (n_frames entries) come back, and
// everything queued is waited for. framesum_api_tx.cpp.
fs_status tx_host_call(fs_ctx* ctx, const uint8_t* src, uint64_t lo, uint64_t hi, uint64_t n_frames, uint64_t frames_bytes,
                       bool gaps, uint8_t* frames, uint64_t* offsets, uint32_t* lengths, fs_digest* out, uint8_t* status,
                       const std::function<fs_status(const TxDevice&)>& enqueue);

// One launch of the context's kernel choice.
// `force` < 0: the context's kernel choice (fs_ctx_set_kernel).
hipError_t launch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                  uint32_t mtu, fs_digest* out, uint8_t* status, hipStream_t stream, FsOp op, uint8_t* wframes,
                  uint32_t tx, int force = -1);

// Grow-only staging of one slot; a slot being regrown first waits for its last kernel.
fs_status ensure_slot(fs_ctx* ctx, HostSlot& sl, uint64_t frame_bytes, uint32_t n);

// A host-staged call that stages its whole batch through slot 0 and runs on the compute stream `ks`
// (fs_fill_batch_host and the four RX host forms): where the batch lies on the device. The
// kernels address frame i at base + offsets[i]: base = staging - cpy_lo (4-B aligned).
struct Staged {
    HostSlot* sl;
    hipStream_t ks;
    uint8_t* base;
    const uint64_t* d_off;
    const uint32_t* d_len;
    fs_digest* d_out;
    uint8_t* d_st;
};
// Behind begin_host_call: the frames' span [lo, hi) (plan::copy_span of it) and the descriptors into
// slot 0, behind the slot's last kernel. Pinned `offsets` and `lengths` (fs_host_alloc, the context's
// mirror) are copied from directly; pageable memory goes through the runtime's own pinned staging.
// The context is dirty from the first copy queued; a later failure drains.
fs_status stage_batch(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, uint64_t lo, uint64_t hi,
                      const uint64_t* offsets, const uint32_t* lengths, uint32_t n, Staged& s);
// ... and behind the call's last enqueue: the slot is marked as read by this call's kernels, and
// everything queued is waited for.
fs_status finish_staged(fs_ctx* ctx, const Staged& s);

}  // namespace host
}  // namespace framesum
