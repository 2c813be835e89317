// stage_layout_test.cpp — mtcp_amd/csrc/stage_layout.hpp on the CPU (no GPU,
// no HIP calls): the layout of every host-memory call's stage buffer over a
// product of batch geometries.  For each call and shape:
//   1. every region's offset meets the alignment its _dev entry checks (the
//      masks stand next to the region names below);
//   2. the regions are in order and disjoint, the back piece is contiguous and
//      covers exactly its regions, the workspace follows at a 16 B boundary and
//      dev_bytes() ends it;
//   3. a bounded HostCall with h_in of exactly in_bytes() and h_out of exactly
//      the out request succeeds (the blocks are heap blocks of exact size:
//      AddressSanitizer sees an overrun by one byte), the inputs arrive at their
//      regions and the caller's outputs receive exactly the bytes the contract
//      names;
//   4. dev_bytes(), back_off(), back_bytes() and every offset equal the values of
//      the hand-chained arithmetic this header replaced, recorded in
//      tests/golden/stage_layout.txt ("call shape | dev_bytes back_off back_bytes
//      h_in h_out | offsets"); the pinned requests lie between what
//      HostCall::take hands out and what that arithmetic asked.
// Built with g++ and run by tests/test_stage_layout_rules.py with the table's
// path; prints one JSON line: per call the number of cases, of failed checks
// and the line of the first one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../mtcp_amd/csrc/stage_layout.hpp"

using namespace mtcp_host;
using mtcp_wait::Deadline;

namespace {

struct Copy {
    uint8_t *dst;
    const uint8_t *src;
    uint64_t bytes;
    bool up;
};
struct FakeDevice {
    std::vector<Copy> queued;
};
struct FakeBackend {
    FakeDevice *d;
    bool copy(void *dst, const void *src, uint64_t bytes, bool up) {
        d->queued.push_back({static_cast<uint8_t *>(dst), static_cast<const uint8_t *>(src), bytes, up});
        return true;
    }
    int drain(int rc) {
        for (const Copy &c : d->queued) memcpy(c.dst, c.src, c.bytes);
        d->queued.clear();
        return rc;
    }
};
using Call = HostCall<FakeBackend>;

constexpr uint8_t kSentinel = 0xA5;

// a heap block of exactly n bytes, 16 B aligned
struct Block {
    uint8_t *p = nullptr;
    uint64_t n;
    Block(uint64_t n_, uint8_t seed, bool pattern) : n(n_) {
        if (n && posix_memalign(reinterpret_cast<void **>(&p), 16, n)) abort();
        for (uint64_t i = 0; i < n; ++i) p[i] = pattern ? (uint8_t)(seed + 7 * i) : seed;
    }
    Block(Block &&o) : p(o.p), n(o.n) { o.p = nullptr; }
    ~Block() { free(p); }
    bool holds(const uint8_t *q, uint64_t len) const { return q >= p && q + len <= p + n; }
};

struct Section {
    const char *name;
    long cases = 0, bad = 0;
    int first_line = 0;
};
Section *cur = nullptr;
#define CHECK(x)                                         \
    do {                                                 \
        if (!(x)) {                                      \
            if (!cur->bad++) cur->first_line = __LINE__; \
        }                                                \
    } while (0)

// the replaced arithmetic's values
struct Golden {
    uint64_t dev_bytes, back_off, back_bytes, h_in, h_out;
    std::vector<uint64_t> offs;
};
std::map<std::string, Golden> golden;

void load_golden(const char *path) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        const size_t bar = line.find(" | ");
        if (bar == std::string::npos) continue;
        std::istringstream in(line.substr(bar + 3));
        Golden g;
        std::string sep;
        in >> g.dev_bytes >> g.back_off >> g.back_bytes >> g.h_in >> g.h_out >> sep;
        for (uint64_t v; in >> v;) g.offs.push_back(v);
        golden[line.substr(0, bar)] = g;
    }
}

// One region of a call: the mask its _dev entry checks (0: a byte pointer),
// what it is used for, and for a back region how many bytes the contract
// hands the caller.  ext: an input that goes elsewhere than the chunk buffer.
struct Row {
    const char *name;
    Region r;
    uint64_t mask;
    unsigned use = 0;
    uint64_t out = 0;
    bool ext = false;
};

std::string key_of(const char *name, std::initializer_list<uint64_t> shape) {
    std::string k = name;
    for (uint64_t v : shape) k += " " + std::to_string(v);
    return k;
}

// The four checks over one layout.  regs: in device order, the workspace last;
// the inputs among them in upload order.  lists: the index in regs of the
// group lists' idx (they go up through up_lists; nlists: four, or six
// with seg_stop and ack_stop), or -1.  image: what comes down pinned before
// the back piece.  two: the results are regs[1] and regs[2] and come down with down2.
void check(const std::string &key, const StageLayout &L, const std::vector<Row> &regs, uint64_t wbytes,
           const GroupLists *g = nullptr, int lists = -1, int nlists = 0, Region image = Region{},
           bool two = false) {
    ++cur->cases;
    // 1, 2
    uint64_t end = 0, back_lo = ~0ull, back_hi = 0;
    bool in_back = false, back_done = false;
    std::vector<uint64_t> offs;
    for (const Row &x : regs) {
        if (x.ext) continue;
        offs.push_back(x.r.off);
        CHECK((x.r.off & x.mask) == 0);
        CHECK(x.r.off >= end);
        end = x.r.off + x.r.bytes;
        if (x.use & kBack) {
            CHECK(!back_done);                              // contiguous: no other region inside
            if (!in_back) back_lo = x.r.off;
            in_back = true;
            back_hi = end;
        } else if (in_back) {
            back_done = true;
        }
    }
    const Region work = regs.back().r;
    CHECK(back_lo == L.back_off && back_hi - back_lo == L.back_bytes());
    CHECK(work.off % 16 == 0 && work.off >= back_hi && work.off - back_hi < 16 && work.bytes == wbytes);
    CHECK(L.dev_bytes == work.off + wbytes);
    // 4
    const auto it = golden.find(key);
    CHECK(it != golden.end());
    if (it == golden.end()) return;
    const Golden &G = it->second;
    CHECK(L.dev_bytes == G.dev_bytes && L.back_off == G.back_off && L.back_bytes() == G.back_bytes);
    CHECK(offs == G.offs);
    // what HostCall::take hands out of h_in and h_out
    uint64_t in_off = 0, in_need = 0;
    for (const Row &x : regs)
        if ((x.use & kIn) && x.r.bytes) {
            in_need = in_off + ((x.use & kStreamed) ? pad16(x.r.bytes) : x.r.bytes);
            in_off += pad16(x.r.bytes);
        }
    const uint64_t out_need = pad16(image.bytes) + L.back_bytes();
    CHECK(in_need <= L.in_bytes && L.in_bytes <= G.h_in);
    CHECK(out_need <= L.out_bytes(image.bytes) && L.out_bytes(image.bytes) <= G.h_out);
    // 3
    Block dev(L.dev_bytes, 11, true), hin(L.in_bytes, 0, false), hout(L.out_bytes(image.bytes), 0, false);
    std::vector<Block> ext, caller;                         // per region: ext device memory, caller memory
    for (size_t i = 0; i < regs.size(); ++i) {
        const Row &x = regs[i];
        ext.emplace_back(x.ext ? x.r.bytes : 0, 0, false);
        if (x.use & kIn) caller.emplace_back(x.r.bytes, (uint8_t)(i + 1), true);
        else caller.emplace_back(x.out, kSentinel, false);
    }
    Stage s;
    s.d_buf = dev.p;
    s.h_in = hin.p, s.h_in_cap = hin.n, s.h_out = hout.p, s.h_out_cap = hout.n;
    FakeDevice fd;
    Call hc(s, Deadline(1000000), {&fd});
    auto u32 = [&](int i) { return reinterpret_cast<const uint32_t *>(caller[i].p); };
    size_t ups = 0;
    for (size_t i = 0; i < regs.size(); ++i) {
        const Row &x = regs[i];
        if ((int)i == lists) {
            const bool stops = nlists == 6 && (regs[i + 4].use & kIn), astop = nlists == 6 && (regs[i + 5].use & kIn);
            if (x.use & kIn)
                g->up(hc, s, u32(i), u32(i + 1), u32(i + 2), u32(i + 3), stops ? u32(i + 4) : nullptr,
                      astop ? u32(i + 5) : nullptr);
            for (int k = 0; k < nlists; ++k) ups += (regs[i + k].use & kIn) && regs[i + k].r.bytes;
            i += nlists - 1;
            continue;
        }
        if (!(x.use & kIn)) continue;
        hc.up(x.ext ? ext[i].p : dev.p + x.r.off, caller[i].p, x.r.bytes, x.use & kStreamed);
        ups += x.r.bytes != 0;
    }
    CHECK(hc.ok() && fd.queued.size() == ups);
    for (const Copy &c : fd.queued) CHECK(c.up && hin.holds(c.src, c.bytes) && (c.src - hin.p) % 16 == 0);
    if (two) {
        // mtcp_gpu_steer's own way down: the pair, adjacent on the device, in one D2H when bounded
        hc.down2(caller[1].p, dev.p + regs[1].r.off, regs[1].r.bytes, caller[2].p, regs[2].r.bytes);
        CHECK(hc.ok() && fd.queued.size() == ups + 1 && fd.queued.back().bytes == L.back_bytes());
        CHECK(!fd.queued.back().up && hout.holds(fd.queued.back().dst, L.back_bytes()));
        CHECK(hc.finish() == MTCP_GPU_OK);
        for (int i = 1; i <= 2; ++i) CHECK(memcmp(caller[i].p, dev.p + regs[i].r.off, regs[i].r.bytes) == 0);
        CHECK(memcmp(ext[0].p, caller[0].p, regs[0].r.bytes) == 0);
        return;
    }
    const uint8_t *himage = hc.down_pinned(dev.p + image.off, image.bytes);
    // fetch: the back piece down, the round finished, and the first result copied out
    size_t first = 0;
    while (first < regs.size() && ((regs[first].use & kIn) || !(regs[first].use & kBack))) ++first;
    const size_t before = fd.queued.size();
    CHECK(first < regs.size() &&
          L.fetch(hc, s, {{caller[first].p, regs[first].r, regs[first].out}}) == MTCP_GPU_OK);
    CHECK(before == ups + (image.bytes != 0) && hout.n >= L.back_bytes());
    const uint8_t *h = hout.p + pad16(image.bytes);         // the slot fetch brought the piece down into
    CHECK(memcmp(h, dev.p + L.back_off, L.back_bytes()) == 0);
    CHECK(!image.bytes || memcmp(himage, dev.p + image.off, image.bytes) == 0);
    for (size_t i = 0; i < regs.size(); ++i) {
        const Row &x = regs[i];
        if ((x.use & kIn) && x.r.bytes)                     // the input arrived whole at its region
            CHECK(memcmp(x.ext ? ext[i].p : dev.p + x.r.off, caller[i].p, x.r.bytes) == 0);
        if ((x.use & kIn) || !(x.use & kBack)) continue;
        CHECK(x.out <= x.r.bytes);
        L.copy_out(h, {{caller[i].p, x.r, x.out}});         // caller[i] holds exactly x.out bytes
        CHECK(!x.out || memcmp(caller[i].p, dev.p + x.r.off, x.out) == 0);
    }
    // a region that goes up and comes back: the caller gets back what the device holds
    for (size_t i = 0; i < regs.size(); ++i)
        if ((regs[i].use & kIn) && (regs[i].use & kBack) && regs[i].r.bytes) {
            Block back(regs[i].r.bytes, kSentinel, false);
            L.copy_out(h, {{back.p, regs[i].r}});
            CHECK(memcmp(back.p, dev.p + regs[i].r.off, back.n) == 0);
        }
}

// the group lists as six regions (rcvwalk and ackwalk have the first four)
void push_lists(std::vector<Row> &v, const GroupLists &g, unsigned in, bool stops, bool ack_stop) {
    v.push_back({"idx", g.idx, 3, in});
    v.push_back({"seg_sid", g.seg_sid, 3, in});
    v.push_back({"seg_start", g.seg_start, 3, in});
    v.push_back({"nseg", g.nseg, 3, in});
    if (!stops) return;
    v.push_back({"seg_stop", g.seg_stop, 3, in});
    v.push_back({"ack_stop", g.ack_stop, 3, ack_stop ? in : 0});
}

const uint32_t kN[] = {1, 3, 4, 5, 256, 257};
const uint32_t kIds[] = {0, 1, 5};
const uint64_t kW[] = {0, 48};

void steer_cases() {
    for (uint32_t n : kN)
        for (uint32_t Q : {1u, 16u})
            for (uint64_t rec : {16ull, 40ull})
                for (uint64_t w : kW) {
                    const SteerLayout l(n, Q, rec, w);
                    check(key_of("steer", {n, Q, rec, w}), l,
                          {{"res", Region{0, n * rec}, 7, kIn, 0, true},
                           {"idx", l.idx, 3, kBack, l.idx.bytes},
                           {"start", l.start, 3, kBack, l.start.bytes},
                           {"work", l.work, 15}},
                          w, nullptr, -1, 0, Region{}, true);
                }
}

void group_cases() {
    for (uint32_t n : kN)
        for (uint64_t w : kW) {
            const GroupLayout l(n, w);
            const uint64_t m = n / 2 + 1;                   // known only on the device: some m <= n
            check(key_of("group", {n, w}), l,
                  {{"sid", l.sid, 3, kIn},
                   {"nseg", l.nseg, 3, kBack, 4},
                   {"idx", l.idx, 3, kBack, l.idx.bytes},
                   {"seg_sid", l.seg_sid, 3, kBack, 4 * m},
                   {"seg_start", l.seg_start, 3, kBack, 4 * m + 4},
                   {"work", l.work, 15}},
                  w);
        }
}

void walk_cases(bool ack) {
    for (uint32_t n : kN)
        for (uint32_t id : kIds)
            for (uint32_t m : {1u, n})
                for (int opt = 0; opt < 2; ++opt)
                    for (uint64_t w : kW) {
                        auto one = [&](const auto &l) {
                            std::vector<Row> v = {{"res", l.res, 7, kIn}, {"opt", l.opt, 15, kIn}};
                            if (ack) v.push_back({"place", l.place, 15, kIn});
                            const int lists = (int)v.size();
                            push_lists(v, l.g, kIn, false, false);
                            v.push_back({ack ? "snd" : "state", l.state, ack ? 127u : 63u, kIn | kBack});
                            v.push_back({ack ? "ack" : "place", l.rec, 15, kBack, l.rec.bytes});
                            v.push_back({ack ? "ack_stop" : "seg_stop", l.stop, 3, kBack, 4ull * m});
                            v.push_back({"work", l.work, 15});
                            check(key_of(ack ? "ackwalk" : "rcvwalk", {n, id, m, (uint64_t)opt, w}), l, v, w, &l.g,
                                  lists, 4);
                        };
                        if (ack) one(AckwalkLayout(n, id, m, opt, true, w));
                        else one(RcvwalkLayout(n, id, m, opt, false, w));
                    }
}

void gen_cases(bool data) {
    for (int i = -1; i < 6; ++i) {
        const uint32_t n = i < 0 ? 0 : kN[i];
        for (uint32_t id : kIds)
            for (uint32_t m : {1u, n}) {
                if (m > n) continue;                        // an empty batch: m = 0 only
                for (int a = 0; a < 2; ++a)                 // ackgen: ack_stop; datagen: ack and ack_stop
                    for (uint32_t sc : {1u, 5u})
                        for (uint64_t w : kW) {
                            auto one = [&](const auto &l) {
                                const unsigned in = n ? kIn : 0;
                                std::vector<Row> v = {{data ? "ack" : "place", l.in_rec, 15, data && !a ? 0 : in}};
                                push_lists(v, l.g, in, true, a);
                                if (data) {
                                    v.push_back({"state", l.state, 63, in});
                                    v.push_back({"snd", l.snd, 127, in | kBack});
                                } else {
                                    v.push_back({"snd", l.snd, 127, in});
                                    v.push_back({"state", l.state, 63, in});
                                }
                                // with n == 0 the states are empty regions of the back piece
                                v.push_back({"tx", l.tx, 31, in | kBack});
                                if (data) v.push_back({"dtx", l.dtx, 15, in | kBack});
                                v.push_back({"seg", l.seg, 7, kBack, l.seg.bytes});
                                v.push_back({"desc", l.desc, 7, kBack, l.desc.bytes});
                                v.push_back({data ? "dres" : "ares", l.res, 15, kBack, 16ull * m});
                                v.push_back({"total", l.total, 7, kBack, 16});
                                v.push_back({"work", l.work, 15});
                                check(key_of(data ? "datagen" : "ackgen", {n, id, m, (uint64_t)a, sc, w}), l, v, w, &l.g,
                                      1, 6);
                            };
                            if (data) one(DatagenLayout(true, n, id, m, a, sc, w));
                            else one(AckgenLayout(false, n, id, m, a, sc, w));
                        }
            }
    }
}

void rto_cases() {
    for (uint32_t id : kIds)
        for (uint32_t cap : {1u, 5u})
            for (uint64_t w : kW) {
                const RtoLayout l(id, cap, w);
                const uint64_t handled = (cap + 1) / 2;     // read from nseg: some count <= cap
                check(key_of("rto", {id, cap, w}), l,
                      {{"snd", l.snd, 127, kIn | kBack},
                       {"dtx", l.dtx, 15, kIn | kBack},
                       {"rto", l.rto, 15, kBack, 16 * handled},
                       {"seg_sid", l.seg_sid, 3, kBack, 4 * handled},
                       {"seg_start", l.seg_start, 3, kBack, l.seg_start.bytes},
                       {"seg_stop", l.seg_stop, 3, kBack, l.seg_stop.bytes},
                       {"nseg", l.nseg, 3, kBack, 4},
                       {"total", l.total, 7, kBack, 16},
                       {"work", l.work, 15}},
                      w);
            }
}

void tx_cases(bool send) {
    for (uint32_t nl : {1u, 3u})
        for (uint64_t pb : {0ull, 1ull, 17ull})
            for (uint64_t bl : {64ull, 65ull}) {
                if (!send) {
                    for (uint32_t n : kN) {
                        const TxLayout l(n, nl, pb, bl);
                        check(key_of("tx_build", {n, nl, pb, bl}), l,
                              {{"image", l.image, 0},
                               {"payload", l.payload, 0, kIn | kStreamed},
                               {"seg", l.seg, 7, kIn},
                               {"links", l.links, 3, kIn},
                               {"desc", Region{0, 8ull * n}, 7, kIn, 0, true},
                               {"status", l.status, 0, kBack, n},
                               {"work", l.work, 15}},
                              0, nullptr, -1, 0, l.image);
                    }
                    continue;
                }
                for (int i = -1; i < 6; ++i)
                    for (uint32_t sc : {1u, 5u})
                        for (uint64_t w : kW) {
                            const uint32_t n = i < 0 ? 0 : kN[i];
                            const TxLayout l(n, nl, pb, bl, sc, w);
                            check(key_of("tx_send", {n, nl, pb, bl, sc, w}), l,
                                  {{"image", l.image, 0},
                                   {"payload", l.payload, 0, kIn | kStreamed},
                                   {"burst", l.burst, 7, kIn},
                                   {"links", l.links, 3, kIn},
                                   {"seg", l.seg, 7},
                                   {"desc", l.desc, 7, kBack, l.desc.bytes},
                                   {"status", l.status, 0, kBack, sc},
                                   {"res", l.res, 7, kBack, l.res.bytes},
                                   {"total", l.total, 7, kBack, 16},
                                   {"work", l.work, 15}},
                                  w, nullptr, -1, 0, l.image);
                        }
            }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    load_golden(argv[1]);
    Section sec[] = {{"steer"}, {"group"}, {"rcvwalk"}, {"ackwalk"}, {"ackgen"}, {"datagen"}, {"rto_sweep"},
                     {"tx_build"}, {"tx_send"}};
    cur = &sec[0], steer_cases();
    cur = &sec[1], group_cases();
    cur = &sec[2], walk_cases(false);
    cur = &sec[3], walk_cases(true);
    cur = &sec[4], gen_cases(false);
    cur = &sec[5], gen_cases(true);
    cur = &sec[6], rto_cases();
    cur = &sec[7], tx_cases(false);
    cur = &sec[8], tx_cases(true);
    printf("{");
    for (size_t i = 0; i < sizeof(sec) / sizeof(sec[0]); ++i)
        printf("%s\"%s\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}", i ? ", " : "", sec[i].name,
               sec[i].cases, sec[i].bad, sec[i].first_line);
    printf("}\n");
    return 0;
}
