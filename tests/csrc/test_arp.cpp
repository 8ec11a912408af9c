// The arithmetic of the ARP call (seqs_amd/csrc/framesum_arp.h) on the CPU, built alone under ASan + UBSan
// by tests/test_arp_host.py: the classification over the grid of one-frame cases (every Operation 0..3, each
// support field off by one, the destination MAC ours, broadcast and one bit away, ProtoTarget and
// ProtoSender ours and one bit away, the query waiting, flagged and absent; frames in heap blocks of exactly
// 42 bytes), both tables under hash masks 0, 0xF and full (lists, key records and tables in heap blocks of
// exactly their size), the slot of a rank and the out records, a built frame's words against bytes put
// together here, its digest sum, every rejection of the two lists with its text, the staged block, and the
// host form's own array description (plan::rx::arp_layout) up to 2^30 frames.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../seqs_amd/csrc/framesum_arp.h"
#include "../../seqs_amd/csrc/framesum_plan.h"

namespace ar = framesum::arp;
namespace fl = framesum::flows;
namespace rxp = framesum::plan::rx;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

static fs_arp_host host(uint32_t i, uint32_t slot0 = 0, uint32_t free_ = 1) {
    fs_arp_host h;
    std::memset(&h, 0, sizeof h);
    h.ip[0] = 10, h.ip[1] = (uint8_t)(i >> 16), h.ip[2] = (uint8_t)(i >> 8), h.ip[3] = (uint8_t)i;
    h.mac[0] = 2, h.mac[1] = 0, h.mac[2] = 0, h.mac[3] = (uint8_t)(i >> 16), h.mac[4] = (uint8_t)(i >> 8), h.mac[5] = (uint8_t)i;
    h.slot0 = slot0, h.free = free_;
    return h;
}
static fs_arp_query query(uint32_t host_index, uint32_t t, uint16_t flags = 0) {
    fs_arp_query q;
    std::memset(&q, 0, sizeof q);
    q.host = host_index;
    q.target[0] = 192, q.target[1] = 168, q.target[2] = (uint8_t)(t >> 8), q.target[3] = (uint8_t)t;
    q.flags = flags;
    return q;
}
// A 42-byte frame in a heap block of exactly its size.
static std::vector<uint8_t> frame(const uint8_t dst[6], uint16_t op, const uint8_t sha[6], const uint8_t spa[4], const uint8_t tha[6],
                                  const uint8_t tpa[4]) {
    std::vector<uint8_t> f(42, 0);
    std::memcpy(&f[0], dst, 6), std::memcpy(&f[6], sha, 6);
    f[12] = 0x08, f[13] = 0x06, f[14] = 0, f[15] = 1, f[16] = 0x08, f[17] = 0, f[18] = 6, f[19] = 4;
    f[20] = (uint8_t)(op >> 8), f[21] = (uint8_t)op;
    std::memcpy(&f[22], sha, 6), std::memcpy(&f[28], spa, 4), std::memcpy(&f[32], tha, 6), std::memcpy(&f[38], tpa, 4);
    return f;
}

// The lists of a call with what check_arp builds and the staged block, every array in a heap block of its size.
struct Lists {
    std::vector<fs_arp_host> hosts;
    std::vector<fs_arp_query> queries;
    ar::Built built;
    std::vector<uint8_t> block;
    ar::Tables t;
    ar::CheckArp build(uint32_t n_reply_slots, uint32_t mask = ~0u, uint32_t flags = 0) {
        const uint32_t nh = (uint32_t)hosts.size(), nq = (uint32_t)queries.size();
        const ar::CheckArp c = ar::check_arp(hosts.data(), nh, queries.data(), nq, n_reply_slots, flags, true, true, true, mask, built);
        if (c.bad != ar::kArpGood) return c;
        const ar::Block b = ar::block_of(nh, nq);
        block.assign(b.bytes, 0xEE);
        ar::stage(hosts.data(), nh, queries.data(), nq, built, b, block.data());
        t = ar::tables_of(block.data(), b, nh, nq, mask);
        return c;
    }
};

static const uint8_t kBroadcast[6] = {255, 255, 255, 255, 255, 255}, kPeerMac[6] = {2, 9, 9, 9, 9, 9}, kZeroMac[6] = {0, 0, 0, 0, 0, 0};

static void test_classify_grid() {
    Lists L;
    L.hosts = {host(1, 0, 2), host(2, 2, 1)};
    L.queries = {query(0, 7), query(0, 8, FS_ARP_SEND_REQUEST), query(1, 7)};
    CHECK(L.build(3).bad == ar::kArpGood);
    const fs_arp_host us = L.hosts[0];
    const uint8_t* target = L.queries[0].target;
    uint32_t seen[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint16_t op = 0; op < 4; ++op)
        for (int dst_kind = 0; dst_kind < 3; ++dst_kind)      // ours, broadcast, one bit away
            for (int tpa_bit = -1; tpa_bit < 32; tpa_bit += 11)  // ours, and one bit away
                for (int spa_kind = 0; spa_kind < 4; ++spa_kind) {  // the waiting query's target, the flagged one's, one bit away, nobody's
                    uint8_t dst[6], tpa[4], spa[4];
                    std::memcpy(dst, dst_kind == 1 ? kBroadcast : us.mac, 6);
                    if (dst_kind == 2) dst[5] ^= 1;
                    std::memcpy(tpa, us.ip, 4);
                    if (tpa_bit >= 0) tpa[tpa_bit >> 3] ^= (uint8_t)(1u << (tpa_bit & 7));
                    std::memcpy(spa, spa_kind == 1 ? L.queries[1].target : target, 4);
                    if (spa_kind == 2) spa[3] ^= 0x80;
                    if (spa_kind == 3) spa[0] = 11;
                    const std::vector<uint8_t> f = frame(dst, op, kPeerMac, spa, kZeroMac, tpa);
                    const ar::Class c = ar::classify(L.t, f.data(), true);
                    uint32_t want = FS_ARP_IGNORED, want_host = ar::kNoArp, want_of = ar::kNoArp;
                    if (op != 1 && op != 2) want = FS_ARP_UNSUPPORTED;
                    else if (dst_kind != 2 && tpa_bit < 0) {
                        if (op == 1) want = FS_ARP_ANSWERED, want_host = 0;
                        else if (spa_kind == 0) want = FS_ARP_STALE, want_of = 0;
                    }
                    CHECK(c.code == want && c.host == want_host && c.of == want_of);
                    ++seen[c.code];
                    CHECK(ar::classify(L.t, nullptr, false).code == FS_ARP_NOT_ARP);
                }
    CHECK(seen[FS_ARP_UNSUPPORTED] && seen[FS_ARP_IGNORED] && seen[FS_ARP_ANSWERED] && seen[FS_ARP_STALE]);
    // each support field off by one, whatever the destination MAC (difference (b))
    for (int at : {15, 17, 18, 19})
        for (int d : {-1, 1})
            for (int foreign = 0; foreign < 2; ++foreign) {
                uint8_t dst[6];
                std::memcpy(dst, us.mac, 6);
                dst[0] ^= (uint8_t)foreign;
                std::vector<uint8_t> f = frame(dst, 1, kPeerMac, target, kZeroMac, us.ip);
                f[at] = (uint8_t)(f[at] + d);
                CHECK(ar::classify(L.t, f.data(), true).code == FS_ARP_UNSUPPORTED);
            }
    for (int at : {14, 16, 20}) {  // the high bytes of the three 16-bit fields
        std::vector<uint8_t> f = frame(us.mac, 2, kPeerMac, target, us.mac, us.ip);
        f[at] = 1;
        CHECK(ar::classify(L.t, f.data(), true).code == FS_ARP_UNSUPPORTED);
    }
    // the second host's query with the same target is its own; with no host nothing matches
    const std::vector<uint8_t> f = frame(kBroadcast, 2, kPeerMac, target, kZeroMac, L.hosts[1].ip);
    CHECK(ar::classify(L.t, f.data(), true).of == 2u);
    const ar::Tables none{};
    CHECK(ar::classify(none, f.data(), true).code == FS_ARP_IGNORED);
    std::vector<uint8_t> bad = f;
    bad[18] = 5;
    CHECK(ar::classify(none, bad.data(), true).code == FS_ARP_UNSUPPORTED);
}

static void test_tables_under_hash_masks() {
    const uint32_t masks[3] = {0u, 0xFu, ~0u};
    for (uint32_t mask : masks)
        for (uint32_t n : {1u, 2u, 3u, 17u, 300u}) {
            Lists L;
            for (uint32_t i = 0; i < n; ++i) L.hosts.push_back(host(i * 256u + 1u, i, 1));
            for (uint32_t i = 0; i < n; ++i) L.queries.push_back(query(i % 3u < n ? i % 3u : 0u, i));
            CHECK(L.build(n, mask).bad == ar::kArpGood);
            CHECK(L.built.htable.size() == fl::table_slots(n) && L.built.qtable.size() == fl::table_slots(n));
            for (uint32_t i = 0; i < n; ++i) {
                CHECK(ar::lookup_host(L.t, ar::le32(L.hosts[i].ip)) == i);
                CHECK(ar::lookup_host(L.t, ar::le32(L.hosts[i].ip) ^ 0x01000000u) == ar::kNoArp);  // the last byte's low bit
                const fs_arp_query& q = L.queries[i];
                CHECK(ar::lookup_query(L.t, ar::le32(L.hosts[q.host].ip), ar::le32(q.target)) == i);
                CHECK(ar::lookup_query(L.t, ar::le32(L.hosts[q.host].ip), ar::le32(q.target) ^ 0x80u) == ar::kNoArp);
                CHECK(ar::lookup_query(L.t, ar::le32(L.hosts[q.host].ip) ^ 2u, ar::le32(q.target)) == ar::kNoArp);
            }
        }
}

static void test_rank_and_out_records() {
    const fs_arp_host h = host(1, 5, 3);
    CHECK(ar::slot_of_rank(h, 0) == 5 && ar::slot_of_rank(h, 2) == 7 && ar::slot_of_rank(h, 3) == ar::kNoArp);
    CHECK(ar::slot_of_rank(host(1, 5, 0), 0) == ar::kNoArp);
    fs_arp_host_out o = ar::host_out(h, 0, ar::kNoArp);
    CHECK(o.n_requests == 0 && o.n_answered == 0 && o.first == ar::kNoArp && o.free == 3);
    o = ar::host_out(h, 2, 9);
    CHECK(o.n_requests == 2 && o.n_answered == 2 && o.first == 9 && o.free == 1);
    o = ar::host_out(h, 70000, 0);
    CHECK(o.n_requests == 70000 && o.n_answered == 3 && o.free == 0);
    const ar::Mac sha = ar::mac_of(kPeerMac);
    fs_arp_query_out q = ar::query_out(query(0, 1), 12, sha, 3);
    CHECK(q.state == FS_ARP_Q_DONE && q.frame == 12 && q.n_replies == 3 && std::memcmp(q.mac, kPeerMac, 6) == 0 && q.reserved == 0);
    q = ar::query_out(query(0, 1), ar::kNoArp, ar::Mac{0, 0}, 0);
    CHECK(q.state == FS_ARP_Q_WAIT && q.frame == ar::kNoArp && q.n_replies == 0 && std::memcmp(q.mac, kZeroMac, 6) == 0);
    q = ar::query_out(query(0, 1, FS_ARP_SEND_REQUEST), 12, sha, 3);  // (a flagged query takes no reply)
    CHECK(q.state == FS_ARP_Q_SENT && q.frame == ar::kNoArp && q.n_replies == 0 && std::memcmp(q.mac, kZeroMac, 6) == 0);
    // the rank key is the UDP call's
    CHECK(ar::rank_port(ar::rank_key(65535, 70000, 17), 17) == 65535 && ar::rank_frame(ar::rank_key(65535, 70000, 17), 17) == 70000);
}

// The 16-bit one's-complement sum the digest has for frame[14:34) (version nibble 4, bytes 24, 25 left out).
static uint32_t ip_csum_bytes(const uint8_t* f) {
    uint32_t s = 0;
    for (int at = 14; at < 34; at += 2) {
        uint32_t hi = f[at], lo = f[at + 1];
        if (at == 14) hi = (hi & 0x0Fu) | 0x40u;
        if (at == 24) hi = lo = 0;
        s += (hi << 8) | lo;
    }
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return ~s & 0xFFFFu;
}

static void test_built_frames() {
    const fs_arp_host h = host(0x010203, 0, 1);
    const uint8_t spa[4] = {192, 168, 7, 9};
    const std::vector<uint8_t> req = frame(kBroadcast, 1, kPeerMac, spa, kZeroMac, h.ip);
    uint32_t w[ar::kFrameWords];
    ar::frame_words(ar::reply_fields(h, ar::parse(req.data())), w);
    uint8_t got[60];
    std::memcpy(got, w, 60);
    std::vector<uint8_t> want = frame(kPeerMac, 2, h.mac, h.ip, kPeerMac, spa);
    want.resize(60, 0);
    CHECK(std::memcmp(got, want.data(), 60) == 0);
    CHECK(ar::ip_csum_of(w) == ip_csum_bytes(want.data()));
    const fs_arp_query q = query(0, 0x0708);
    ar::frame_words(ar::request_fields(h, q), w);
    std::memcpy(got, w, 60);
    want = frame(kBroadcast, 1, h.mac, h.ip, kZeroMac, q.target);
    want.resize(60, 0);
    CHECK(std::memcmp(got, want.data(), 60) == 0);
    CHECK(ar::ip_csum_of(w) == ip_csum_bytes(want.data()));
    CHECK(ar::frame_len(0) == 42 && ar::frame_len(FS_ARP_PAD) == 60 && ar::frame_len(FS_FCS_APPEND) == 42);
    CHECK(ar::built_verdict(42, 0) == FS_ARP && ar::built_verdict(42, 42) == FS_ARP && ar::built_verdict(60, 59) == FS_ERR_EXCEEDS_MTU);
}

static void test_rejections() {
    struct Case {
        void (*change)(Lists&);
        ar::BadArp bad;
        uint32_t index;
        const char* text;
    };
    const Case cases[] = {
        {[](Lists& L) { L.hosts[1].reserved = 1; }, ar::kHostReserved, 1, "a host's reserved must be 0"},
        {[](Lists& L) { std::memcpy(L.hosts[2].ip, L.hosts[0].ip, 4); }, ar::kEqualIp, 2, "its ip equals an earlier host's"},
        {[](Lists& L) { L.hosts[2].free = 3; }, ar::kArpSlotRange, 2, "its slot range ends past n_reply_slots"},
        {[](Lists& L) { L.hosts[2].slot0 = 7; L.hosts[2].free = 0; }, ar::kArpSlotRange, 2, "its slot range ends past n_reply_slots"},
        {[](Lists& L) { L.hosts[1].slot0 = 1; }, ar::kArpSlotsOverlap, 1, "its slot range overlaps another host's"},
        {[](Lists& L) { L.queries[1].host = 3; }, ar::kQueryHost, 1, "its host is not below n_hosts"},
        {[](Lists& L) { L.queries[1] = L.queries[0]; }, ar::kEqualQuery, 1, "its host and target equal an earlier query's"},
        {[](Lists& L) { L.queries[0].flags = 2; }, ar::kQueryFlags, 0, "its flags must be 0 or FS_ARP_SEND_REQUEST"},
        {[](Lists& L) { L.queries[1].reserved = 1; }, ar::kQueryReserved, 1, "a query's reserved must be 0"},
    };
    for (const Case& c : cases)
        for (uint32_t mask : {0u, ~0u}) {
            Lists L;
            L.hosts = {host(1, 0, 2), host(2, 2, 2), host(3, 4, 2)};
            L.queries = {query(0, 1), query(0, 2), query(2, 1)};
            CHECK(L.build(6, mask).bad == ar::kArpGood);
            c.change(L);
            const ar::CheckArp got = L.build(6, mask);
            CHECK(got.bad == c.bad && got.index == c.index && std::string(ar::bad_arp_text(got.bad)) == c.text);
        }
    // the call's own numbers and pointers
    Lists L;
    L.hosts = {host(1)};
    L.queries = {query(0, 1)};
    ar::Built b;
    const auto check = [&](uint32_t nh, uint32_t nq, uint32_t slots, uint32_t flags, bool ho, bool qo, bool fr, const fs_arp_host* hp,
                           const fs_arp_query* qp) { return ar::check_arp(hp, nh, qp, nq, slots, flags, ho, qo, fr, ~0u, b).bad; };
    const fs_arp_host* hp = L.hosts.data();
    const fs_arp_query* qp = L.queries.data();
    CHECK(check(1, 1, 1, 3, true, true, true, hp, qp) == ar::kArpGood);
    CHECK(check(65537, 0, 1, 0, true, true, true, hp, qp) == ar::kTooManyHosts);
    CHECK(check(1, 65537, 1, 0, true, true, true, hp, qp) == ar::kTooManyQueries);
    CHECK(check(1, 1, 65537, 0, true, true, true, hp, qp) == ar::kTooManyReplySlots);
    CHECK(check(1, 1, 1, 4, true, true, true, hp, qp) == ar::kArpFlagsBad);
    CHECK(check(1, 0, 1, 0, true, true, true, nullptr, qp) == ar::kArpNullHosts);
    CHECK(check(1, 0, 1, 0, false, true, true, hp, qp) == ar::kArpNullHosts);
    CHECK(check(1, 0, 1, 0, true, true, false, hp, qp) == ar::kArpNullHosts);
    CHECK(check(1, 1, 1, 0, true, true, true, hp, nullptr) == ar::kArpNullQueries);
    CHECK(check(1, 1, 1, 0, true, false, true, hp, qp) == ar::kArpNullQueries);
    CHECK(check(0, 1, 0, 0, true, true, true, nullptr, qp) == ar::kQueryHost);  // a query names a host
    CHECK(check(0, 0, 0, 0, false, false, false, nullptr, nullptr) == ar::kArpGood);
    for (int k = ar::kArpNullHosts; k <= ar::kQueryFlags; ++k) CHECK(std::strlen(ar::bad_arp_text((ar::BadArp)k)) > 0);
    // 65,536 hosts of one slot each and as many queries are good
    Lists big;
    for (uint32_t i = 0; i < 65536u; ++i) big.hosts.push_back(host(i, i, 1)), big.queries.push_back(query(i, i & 0xFFFFu));
    CHECK(big.build(65536).bad == ar::kArpGood);
    CHECK(ar::lookup_host(big.t, ar::le32(big.hosts[65535].ip)) == 65535u);
}

static void test_staged_block() {
    for (uint32_t nh : {1u, 3u, 300u})
        for (uint32_t nq : {0u, 1u, 5u}) {
            const ar::Block b = ar::block_of(nh, nq);
            CHECK(b.queries == 20ull * nh && b.htable == b.queries + 12ull * nq && b.htable % 4 == 0 && b.qtable % 4 == 0);
            CHECK(b.hkeys == b.qtable + 4ull * fl::table_slots(nq) && b.qkeys == b.hkeys + 13ull * nh && b.bytes == b.qkeys + 13ull * nq);
        }
}

static void test_host_form_layout() {
    CHECK(rxp::kArp == rxp::kUdp + 1);
    for (uint64_t n : {0ull, 1ull, 3ull, 65793ull, 1ull << 30})
        for (uint64_t nh : {0ull, 1ull, 65536ull})
            for (uint64_t nq : {0ull, 3ull, 65536ull})
                for (uint64_t base : {0ull, 1ull, 13ull}) {
                    const uint64_t slots = nh + nq;
                    const rxp::ArpLayout L = rxp::arp_layout(base, rxp::ArpCounts{{nh, nq, slots, n}});
                    uint64_t at = base;
                    for (uint32_t a = 0; a < rxp::kArpArrays; ++a) {
                        const rxp::ArpArrayDesc& d = rxp::kArpArrayDesc[a];
                        CHECK(L.at[a] >= at && L.at[a] % d.align == 0 && L.at[a] - at < d.align);
                        const uint64_t count = d.count == rxp::kPerHost ? nh : d.count == rxp::kPerQuery ? nq : d.count == rxp::kPerFrameSlot ? slots : n;
                        CHECK(L.room[a] == d.elem * count);
                        at = L.at[a] + L.room[a];
                    }
                    CHECK(L.bytes == at);
                }
    CHECK(rxp::kArpArrayDesc[rxp::kHostsOut].elem == sizeof(fs_arp_host_out) && rxp::kArpArrayDesc[rxp::kQueriesOut].elem == sizeof(fs_arp_query_out));
    CHECK(rxp::kArpArrayDesc[rxp::kArpFrames].elem == FS_ACCEPT_STRIDE && rxp::kArpArrayDesc[rxp::kArpOut].elem == sizeof(fs_digest));
    CHECK(rxp::kArpArrayDesc[rxp::kArpFrames].goes_in && rxp::kArpArrayDesc[rxp::kArpOut].goes_in && rxp::kArpArrayDesc[rxp::kArpStatus].goes_in);
    CHECK(!rxp::kArpArrayDesc[rxp::kArpCode].goes_in && !rxp::kArpArrayDesc[rxp::kArpOf].goes_in);
    // the ninth kind has every array of the kinds before it
    const rxp::Layout a = rxp::layout(rxp::kArp, 1ull << 30, 7), u = rxp::layout(rxp::kUdp, 1ull << 30, 7);
    CHECK(a.bytes == u.bytes && rxp::totals_bytes(rxp::kArp) == 24);
    for (uint32_t k = 0; k < rxp::kArrays; ++k) CHECK(a.at[k] == u.at[k] && a.room[k] == u.room[k]);
}

int main() {
    test_classify_grid();
    test_tables_under_hash_masks();
    test_rank_and_out_records();
    test_built_frames();
    test_rejections();
    test_staged_block();
    test_host_form_layout();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("arp checks OK\n");
    return 0;
}
