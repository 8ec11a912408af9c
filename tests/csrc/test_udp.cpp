// The arithmetic of the UDP call (seqs_amd/csrc/framesum_udp.h) on the CPU, built alone under ASan + UBSan
// by tests/test_udp_host.py: the match over every byte of a key record, the port table under hash masks
// 0, 0xF and full (tables and port lists in heap blocks of exactly their size), the wildcard as the second
// probe, the rank key, admission and wrap, every rejection of the port list with its text, the datagram's
// numbers and the cell header at every truncation (frames in heap blocks of exactly their size), the
// staged block, and the host form's own array description (plan::rx::udp_layout) up to 2^30 frames.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../seqs_amd/csrc/framesum_plan.h"
#include "../../seqs_amd/csrc/framesum_udp.h"

namespace ud = framesum::udp;
namespace fl = framesum::flows;
namespace ac = framesum::accept;
namespace rxp = framesum::plan::rx;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

static fs_udp_port port(uint32_t i, uint32_t n_cells = 4, uint32_t cell_size = 64) {
    fs_udp_port p;
    std::memset(&p, 0, sizeof p);
    p.local[0] = 10, p.local[1] = (uint8_t)(i >> 16), p.local[2] = (uint8_t)(i >> 8), p.local[3] = (uint8_t)i;
    p.local[4] = (uint8_t)((i * 7u + 1u) >> 8), p.local[5] = (uint8_t)((i * 7u + 1u) | 1u);
    p.n_cells = n_cells, p.cell_size = cell_size, p.cells_off = (uint64_t)i * n_cells * cell_size;
    p.wcell = 0, p.free = n_cells;
    return p;
}
// The key record of an accepted frame of protocol `proto` from anywhere to `local`.
static fl::Key key_to(const uint8_t local[6], uint8_t proto = 17) {
    uint8_t k[13] = {proto, 192, 168, 1, 77, local[0], local[1], local[2], local[3], 0x30, 0x39, local[4], local[5]};
    return fl::wire_key(k);
}

static void test_match_over_every_key_byte() {
    std::vector<fs_udp_port> ports{port(1), port(2)};
    std::vector<uint32_t> table(fl::table_slots(2));
    CHECK(ud::build_port_table(ports.data(), 2, ~0u, table.data()) == fl::kEmpty);
    const uint32_t tmask = (uint32_t)table.size() - 1u;
    const fl::Key good = key_to(ports[1].local);
    CHECK(ud::match_port(good, ports.data(), table.data(), 2, tmask, ~0u) == 1u);
    for (uint32_t byte = 0; byte < 16; ++byte)
        for (uint32_t bit = 0; bit < 8; ++bit) {
            fl::Key k = good;
            k.w[byte >> 2] ^= 1u << (8u * (byte & 3u) + bit);
            const uint32_t got = ud::match_port(k, ports.data(), table.data(), 2, tmask, ~0u);
            // the source (bytes 1..4, 9, 10) and the unused bytes 13, 14 do not matter; the protocol, the
            // destination and the accepted bit (byte 15, bit 0) do
            const bool matters = byte == 0 || (byte >= 5 && byte <= 8) || byte == 11 || byte == 12 || (byte == 15 && bit == 0);
            CHECK(got == (matters ? ud::kNoPort : 1u));
        }
    CHECK(ud::match_port(key_to(ports[1].local, 6), ports.data(), table.data(), 2, tmask, ~0u) == ud::kNoPort);
    CHECK(ud::match_port(fl::no_key(), ports.data(), table.data(), 2, tmask, ~0u) == ud::kNoPort);
    CHECK(ud::match_port(good, nullptr, nullptr, 0, 1, ~0u) == ud::kNoPort);
}

static void test_table_under_hash_masks() {
    const uint32_t masks[3] = {0u, 0xFu, ~0u};
    for (uint32_t mask : masks)
        for (uint32_t n : {1u, 2u, 3u, 17u, 300u}) {
            // heap blocks of exactly their size: a probe past either end is a sanitizer report
            fs_udp_port* ports = (fs_udp_port*)std::malloc(sizeof(fs_udp_port) * n);
            for (uint32_t i = 0; i < n; ++i) ports[i] = port(i + 1);
            // the last port is the wildcard for port[0]'s number
            if (n > 1) std::memset(ports[n - 1].local, 0, 4), ports[n - 1].local[4] = ports[0].local[4], ports[n - 1].local[5] = ports[0].local[5];
            const uint32_t slots = fl::table_slots(n);
            uint32_t* table = (uint32_t*)std::malloc(4u * slots);
            CHECK(ud::build_port_table(ports, n, mask, table) == fl::kEmpty);
            for (uint32_t i = 0; i < n; ++i) {
                if (n > 1 && i == n - 1) continue;
                CHECK(ud::match_port(key_to(ports[i].local), ports, table, n, slots - 1u, mask) == i);
            }
            if (n > 1) {  // another address with port[0]'s number: the wildcard; port[0]'s own address: port[0]
                uint8_t other[6] = {172, 16, 0, 9, ports[0].local[4], ports[0].local[5]};
                CHECK(ud::match_port(key_to(other), ports, table, n, slots - 1u, mask) == n - 1u);
                uint8_t zero[6] = {0, 0, 0, 0, ports[0].local[4], ports[0].local[5]};
                CHECK(ud::match_port(key_to(zero), ports, table, n, slots - 1u, mask) == n - 1u);
                uint8_t nobody[6] = {172, 16, 0, 9, 0xEE, 0xEE};
                CHECK(ud::match_port(key_to(nobody), ports, table, n, slots - 1u, mask) == ud::kNoPort);
            }
            std::free(table);
            std::free(ports);
        }
}

static void test_rank_and_admission() {
    for (uint32_t n : {1u, 255u, 65793u, 1u << 30}) {
        const uint32_t b = fl::index_bits(n);
        for (uint32_t n_ports : {1u, 2u, 1000u, 65536u}) {
            const uint32_t bits = ac::rank_bits(b, n_ports);
            CHECK(bits <= 48u);
            const uint64_t mask = ((uint64_t)1 << bits) - 1u;
            const uint64_t k = ac::rank_key(n_ports - 1u, n - 1u, b);
            CHECK(ud::rank_port(k, b) == n_ports - 1u && ud::rank_frame(k, b) == n - 1u);
            CHECK((k & mask) == k && (ud::kUnmatched & mask) > k);  // an unmatched frame sorts behind every port's
        }
    }
    fs_udp_port p = port(0, 5);
    p.wcell = 4, p.free = 3;
    CHECK(ud::cell_of_rank(p, 0) == 4u && ud::cell_of_rank(p, 1) == 0u && ud::cell_of_rank(p, 2) == 1u);
    CHECK(ud::cell_of_rank(p, 3) == ud::kCellFull && ud::cell_of_rank(p, 0xFFFFFFFFu) == ud::kCellFull);
    fs_udp_port_out o = ud::port_out(p, 7);
    CHECK(o.n_matched == 7u && o.n_admitted == 3u && o.wcell == 2u && o.free == 0u && o.first == ud::kNoPort && o.bytes == 0u);
    o = ud::port_out(p, 0);
    CHECK(o.n_matched == 0u && o.n_admitted == 0u && o.wcell == 4u && o.free == 3u);
    fs_udp_port big = port(0, 1u << 31, 40);
    big.wcell = (1u << 31) - 1u, big.free = 1u << 31;
    CHECK(ud::cell_of_rank(big, 0) == (1u << 31) - 1u && ud::cell_of_rank(big, 1) == 0u);
    CHECK(ud::port_out(big, 0xFFFFFFFFu).wcell == (1u << 31) - 1u && ud::port_out(big, 0xFFFFFFFFu).free == 0u);
    fs_udp_port one = port(0, 1);
    CHECK(ud::cell_of_rank(one, 0) == 0u && ud::cell_of_rank(one, 1) == ud::kCellFull && ud::port_out(one, 2).wcell == 0u);
}

static void test_every_rejection() {
    std::vector<uint32_t> table;
    const auto bad = [&](std::vector<fs_udp_port> ports, uint64_t cells_bytes = 1u << 20, bool cells = true, bool out = true) {
        return ud::check_ports(ports.data(), (uint32_t)ports.size(), cells, out, cells_bytes, ~0u, table);
    };
    std::vector<fs_udp_port> good{port(0), port(1), port(2)};
    ud::CheckUdp c = bad(good);
    CHECK(c.bad == ud::kUdpGood && c.lo == 0 && c.hi == 3u * 4u * 64u && table.size() == fl::table_slots(3));
    CHECK(bad({}).bad == ud::kUdpGood && bad({}, 0, false, false).bad == ud::kUdpGood);
    CHECK(ud::check_ports(nullptr, 1, true, true, 64, ~0u, table).bad == ud::kUdpNull);
    CHECK(bad(good, 1u << 20, false).bad == ud::kUdpNull && bad(good, 1u << 20, true, false).bad == ud::kUdpNull);
    CHECK(ud::check_ports(good.data(), ud::kMaxPorts + 1u, true, true, 64, ~0u, table).bad == ud::kTooManyPorts);
    const auto with = [&](void (*change)(fs_udp_port&)) {
        std::vector<fs_udp_port> ports = good;
        change(ports[1]);
        return ports;
    };
    c = bad(with([](fs_udp_port& p) { p.reserved[1] = 1; }));
    CHECK(c.bad == ud::kUdpReserved && c.index == 1u);
    CHECK(bad(with([](fs_udp_port& p) { p.local[4] = p.local[5] = 0; })).bad == ud::kUdpZeroPort);
    CHECK(bad(with([](fs_udp_port& p) { std::memcpy(p.local, "\x0a\0\0\0\0\1", 6); })).bad == ud::kUdpEqualLocal);
    for (uint32_t size : {0u, 32u, 39u, 44u, 65569u, 65576u}) {
        std::vector<fs_udp_port> ports = good;
        ports[1].cell_size = size;
        CHECK(bad(ports).bad == ud::kUdpCellSize);
    }
    for (uint32_t size : {40u, 48u, 65568u}) {
        std::vector<fs_udp_port> ports{port(0, 1, size)};
        CHECK(bad(ports).bad == ud::kUdpGood);
    }
    CHECK(bad(with([](fs_udp_port& p) { p.cells_off += 4; })).bad == ud::kUdpCellsOff);
    CHECK(bad(with([](fs_udp_port& p) { p.n_cells = 0; })).bad == ud::kUdpNCells);
    CHECK(bad(with([](fs_udp_port& p) { p.n_cells = (1u << 31) + 1u; })).bad == ud::kUdpNCells);
    CHECK(bad(with([](fs_udp_port& p) { p.wcell = p.n_cells; })).bad == ud::kUdpWcell);
    CHECK(bad(with([](fs_udp_port& p) { p.free = p.n_cells + 1u; })).bad == ud::kUdpFree);
    CHECK(bad(good, 3u * 256u - 1u).bad == ud::kUdpOutside && bad(good, 3u * 256u).bad == ud::kUdpGood);
    CHECK(bad(with([](fs_udp_port& p) { p.cells_off = ~(uint64_t)7; })).bad == ud::kUdpOutside);
    c = bad(with([](fs_udp_port& p) { p.cells_off -= 8; }));
    CHECK(c.bad == ud::kUdpOverlap && c.index == 1u);
    c = bad(with([](fs_udp_port& p) { p.cells_off += 8; }));
    CHECK(c.bad == ud::kUdpOverlap && c.index == 2u);
    CHECK(bad(with([](fs_udp_port& p) { p.cells_off = 0; })).bad == ud::kUdpOverlap);
    {  // a 2^31-cell queue of the largest cells is in range where cells_bytes allows it
        std::vector<fs_udp_port> ports{port(0, 1u << 31, 65568)};
        ports[0].cells_off = 8;
        CHECK(bad(ports, ~(uint64_t)0).bad == ud::kUdpGood && bad(ports, ((uint64_t)65568 << 31) + 7u).bad == ud::kUdpOutside);
    }
    for (int b = ud::kUdpNull; b <= ud::kUdpOverlap; ++b) CHECK(std::strlen(ud::bad_udp_text((ud::BadUdp)b)) > 0);
    CHECK(std::strlen(ud::bad_udp_text(ud::kUdpGood)) == 0);
}

// A UDP frame with `ihl` header words and `len` payload bytes in a heap block of exactly its size.
static uint8_t* frame_of(uint32_t ihl, uint32_t len, uint32_t& size, uint32_t udp_length_delta = 0) {
    const uint32_t l4 = 14u + 4u * ihl;
    size = l4 + 8u + len;
    uint8_t* f = (uint8_t*)std::malloc(size);
    for (uint32_t i = 0; i < size; ++i) f[i] = (uint8_t)(i * 13u + 5u);
    f[14] = (uint8_t)(0x40u | ihl);
    const uint32_t total = 4u * ihl + 8u + len;
    f[16] = (uint8_t)(total >> 8), f[17] = (uint8_t)total;
    f[23] = 17;
    const uint32_t ulen = 8u + len + udp_length_delta;
    f[l4] = 0x12, f[l4 + 1] = 0x34, f[l4 + 2] = 0, f[l4 + 3] = 67, f[l4 + 4] = (uint8_t)(ulen >> 8), f[l4 + 5] = (uint8_t)ulen;
    return f;
}

static void test_cell_writer_at_every_truncation() {
    for (uint32_t ihl : {5u, 6u, 15u})
        for (uint32_t cell_size : {40u, 48u, 64u, 1504u})
            for (uint32_t len = 0; len <= cell_size - 32u + 2u; ++len) {
                uint32_t size;
                uint8_t* f = frame_of(ihl, len, size, len & 1u);
                const ud::Dgram d = ud::dgram_of(f, size, cell_size);
                const uint32_t room = cell_size - 32u;
                CHECK(d.start == 14u + 4u * ihl + 8u && d.len == len && d.stored == (len < room ? len : room));
                CHECK(d.udp_length == 8u + len + (len & 1u) && d.src_port == 0x1234u);
                uint32_t w[8];
                ud::cell_words(f, 0xA0B0C0D0u + len, d, w);
                fs_udp_cell c;
                std::memcpy(&c, w, 32);
                CHECK(c.frame == 0xA0B0C0D0u + len && c.len == len && c.stored == d.stored && c.udp_length == d.udp_length);
                CHECK(c.src_port == 0x1234u && !std::memcmp(c.src_ip, f + 26, 4) && !std::memcmp(c.dst_ip, f + 30, 4));
                CHECK(!std::memcmp(c.src_mac, f + 6, 6) && !std::memcmp(c.dst_mac, f, 6));
                // a frame cut short by a caller's mistake: never more than the frame holds
                if (len > 0) CHECK(ud::dgram_of(f, size - 1u, cell_size).stored <= len - 1u);
                // the key record from the frame's own bytes is the one the flow stage makes
                const fl::Key k = ud::key_of_frame(f, true);
                CHECK(ud::is_datagram(k) && fl::key_byte(k, 11) == 0u && fl::key_byte(k, 12) == 67u && fl::key_byte(k, 5) == f[30]);
                CHECK(!ud::is_datagram(ud::key_of_frame(f, false)));
                std::free(f);
            }
    {  // the largest datagram: 65,507 bytes into the largest cell
        uint32_t size;
        uint8_t* f = frame_of(5, 65507, size);
        CHECK(ud::dgram_of(f, size, 65568).stored == 65507u && ud::dgram_of(f, size, 65568).len == 65507u);
        CHECK(ud::dgram_of(f, size, 40).stored == 8u);
        std::free(f);
    }
}

static void test_block_and_layout() {
    std::vector<fs_udp_port> ports{port(0), port(1), port(2)};
    std::vector<uint32_t> table;
    CHECK(ud::check_ports(ports.data(), 3, true, true, 1u << 20, 0xFu, table).bad == ud::kUdpGood);
    const ud::Block b = ud::block_of(3);
    CHECK(b.table == 96u && b.bytes == 96u + 4u * fl::table_slots(3));
    uint8_t* dst = (uint8_t*)std::malloc(b.bytes);
    ud::stage(ports.data(), 3, table.data(), b, dst);
    CHECK(!std::memcmp(dst, ports.data(), 96) && !std::memcmp(dst + 96, table.data(), b.bytes - 96));
    std::free(dst);
    const ud::Block none = ud::block_of(0);
    CHECK(none.table == 0 && none.bytes == 4u * fl::table_slots(0));
    // the host form's own arrays behind the others': aligned, disjoint, in order, up to 2^30 frames
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)65793, (uint64_t)1 << 30})
        for (uint64_t n_ports : {(uint64_t)0, (uint64_t)1, (uint64_t)65536})
            for (uint64_t base : {(uint64_t)0, (uint64_t)1, (uint64_t)4099}) {
                const rxp::UdpLayout L = rxp::udp_layout(base, n, n_ports);
                uint64_t at = base;
                for (uint32_t a = 0; a < rxp::kUdpArrays; ++a) {
                    CHECK(L.at[a] >= at && L.at[a] < at + rxp::kUdpArrayDesc[a].align && L.at[a] % rxp::kUdpArrayDesc[a].align == 0);
                    at = L.at[a] + L.room[a];
                }
                CHECK(L.bytes == at && L.room[rxp::kPortsOut] == 32u * n_ports && L.room[rxp::kPortOf] == 4u * n &&
                      L.room[rxp::kCellOf] == 4u * n);
            }
    CHECK(rxp::kUdp == rxp::kConnect + 1 && rxp::totals_bytes(rxp::kUdp) == 24 && rxp::layout(rxp::kUdp, 7, 3).bytes == rxp::layout(rxp::kConnect, 7, 3).bytes);
}

int main() {
    test_match_over_every_key_byte();
    test_table_under_hash_masks();
    test_rank_and_admission();
    test_every_rejection();
    test_cell_writer_at_every_truncation();
    test_block_and_layout();
    if (g_failed) {
        std::printf("%d udp checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("udp checks OK\n");
    return 0;
}
