// host_call_test.cpp — mtcp_amd/csrc/host_call.hpp on the CPU (no GPU, no
// HIP calls): the wait-limit contract of the host-memory calls, checked on
// the addresses the queued copies name and on when caller memory is written.
// The backend records every queued copy and performs it only when drained;
// the "device" and the stage's h_in / h_out are heap blocks of exact size, so
// that AddressSanitizer sees an overrun by one byte.  Built with g++ and run
// by tests/test_host_call_rules.py; prints one JSON line: per section the
// number of cases, of failed checks and the line of the first one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mtcp_amd/csrc/host_call.hpp"

using mtcp_host::HostCall;
using mtcp_host::Stage;
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
    size_t ran = 0;              // copies performed so far
    int calls = 0, fail_at = -1; // the fail_at-th copy (from 0) is refused
    bool stalled = false;        // drain answers MTCP_GPU_ETIMEDOUT and runs nothing
    bool abandoned = false;
    int drains = 0;
    void run() {
        for (; ran < queued.size(); ++ran) memcpy(queued[ran].dst, queued[ran].src, queued[ran].bytes);
    }
};

struct FakeBackend {
    FakeDevice *d;
    bool copy(void *dst, const void *src, uint64_t bytes, bool up) {
        if (d->calls++ == d->fail_at) return false;
        d->queued.push_back({static_cast<uint8_t *>(dst), static_cast<const uint8_t *>(src), bytes, up});
        return true;
    }
    int drain(int rc) {
        ++d->drains;
        if (d->stalled) {
            d->abandoned = true;
            return MTCP_GPU_ETIMEDOUT;
        }
        d->run();
        return rc;
    }
};
using Call = HostCall<FakeBackend>;

constexpr uint8_t kSentinel = 0xA5;   // the caller's outputs before a call
constexpr uint8_t kPinned = 0x5A;     // h_in / h_out before a call: a copy-out of stale staging shows

// a heap block of exactly n bytes, 16 B aligned, filled with `fill`
struct Block {
    uint8_t *p = nullptr;
    uint64_t n;
    Block(uint64_t n_, uint8_t fill) : n(n_) {
        if (n && posix_memalign(reinterpret_cast<void **>(&p), 16, n)) abort();
        if (n) memset(p, fill, n);
    }
    ~Block() { free(p); }
    Block(const Block &) = delete;
    bool all(uint8_t v) const {
        for (uint64_t i = 0; i < n; ++i)
            if (p[i] != v) return false;
        return true;
    }
    bool holds(const void *q) const { return n && q >= p && q < p + n; }
    bool pattern(uint8_t seed) const {
        for (uint64_t i = 0; i < n; ++i)
            if (p[i] != (uint8_t)(seed + 3 * i)) return false;
        return true;
    }
    void set_pattern(uint8_t seed) {
        for (uint64_t i = 0; i < n; ++i) p[i] = (uint8_t)(seed + 3 * i);
    }
};

uint64_t pad(uint64_t v) { return (v + 15) & ~15ull; }

struct Section {
    const char *name;
    long cases = 0, bad = 0;
    int first_line = 0;
};
Section *cur = nullptr;
#define CHECK(x)                                      \
    do {                                              \
        if (!(x)) {                                   \
            if (!cur->bad++) cur->first_line = __LINE__; \
        }                                             \
    } while (0)

// the caller's two inputs and two outputs, the device's copies of them, and a
// stage whose h_in / h_out hold exactly what a bounded call bounces
struct Fixture {
    Block a, b, x, y;            // caller memory
    Block da, db, dx, dy;        // device memory
    Block hin, hout;
    Stage s;
    FakeDevice dev;
    Fixture(uint64_t la, uint64_t lb, uint64_t lx, uint64_t ly, bool a_streamed = false)
        : a(la, 0), b(lb, 0), x(lx, kSentinel), y(ly, kSentinel), da(la, 0), db(lb, 0), dx(lx, 0), dy(ly, 0),
          hin(lb || a_streamed ? pad(la) + lb : la, kPinned), hout(ly ? pad(lx) + ly : lx, kPinned) {
        a.set_pattern(1);
        b.set_pattern(2);
        dx.set_pattern(3);       // what a kernel left on the device
        dy.set_pattern(4);
        s.h_in = hin.p;
        s.h_in_cap = hin.n;
        s.h_out = hout.p;
        s.h_out_cap = hout.n;
    }
    bool caller_holds(const void *q) const { return a.holds(q) || b.holds(q) || x.holds(q) || y.holds(q); }
    bool outputs_untouched() const { return x.all(kSentinel) && y.all(kSentinel); }
    bool outputs_correct() const { return x.pattern(3) && y.pattern(4); }
    bool inputs_arrived() const { return da.pattern(1) && db.pattern(2); }
};

const uint64_t kLens[] = {0, 1, 15, 16, 17};

void up_and_down(Call &hc, Fixture &f, bool a_streamed) {
    hc.up(f.da.p, f.a.p, f.a.n, a_streamed);
    hc.up(f.db.p, f.b.p, f.b.n);
    hc.down(f.x.p, f.dx.p, f.x.n);
    hc.down(f.y.p, f.dy.p, f.y.n);
}

// 1. unbounded: the copies name the caller's own pointers, the bounce buffers stay untouched
void unbounded(uint64_t la, uint64_t lb, uint64_t lx, uint64_t ly) {
    Fixture f(la, lb, lx, ly);
    Call hc(f.s, Deadline(0), {&f.dev});
    up_and_down(hc, f, la & 1);
    const Copy want[] = {{f.da.p, f.a.p, la, true}, {f.db.p, f.b.p, lb, true},
                         {f.x.p, f.dx.p, lx, false}, {f.y.p, f.dy.p, ly, false}};
    size_t k = 0;
    for (const Copy &w : want) {
        if (!w.bytes) continue;                       // nothing to queue
        CHECK(k < f.dev.queued.size());
        if (k >= f.dev.queued.size()) break;
        const Copy &c = f.dev.queued[k++];
        CHECK(c.dst == w.dst && c.src == w.src && c.bytes == w.bytes && c.up == w.up);
    }
    CHECK(k == f.dev.queued.size());
    CHECK(f.outputs_untouched());
    CHECK(hc.finish() == MTCP_GPU_OK);
    CHECK(f.outputs_correct() && f.inputs_arrived());
    CHECK(f.hin.all(kPinned) && f.hout.all(kPinned));
    CHECK(f.s.npend == 0 && !f.dev.abandoned);
    // down_pinned lands in h_out in either mode
    const uint8_t *pin = hc.down_pinned(f.dx.p, lx);
    CHECK(lx == 0 || (f.dev.queued.back().dst == f.hout.p && pin == f.hout.p));
    CHECK(hc.finish() == MTCP_GPU_OK && (lx == 0 || memcmp(pin, f.dx.p, lx) == 0));
}

// 2. bounded: no queued copy names caller memory; 16 B aligned slots that do not overlap;
//    the caller's outputs are written by finish() alone
void bounded(uint64_t la, uint64_t lb, uint64_t lx, uint64_t ly) {
    const bool a_streamed = la & 1;
    Fixture f(la, lb, lx, ly, a_streamed);
    Call hc(f.s, Deadline(1000000), {&f.dev});
    up_and_down(hc, f, a_streamed);
    CHECK(hc.ok());
    const uint8_t *in_end = f.hin.p, *out_end = f.hout.p;
    for (const Copy &c : f.dev.queued) {
        CHECK(!f.caller_holds(c.dst) && !f.caller_holds(c.src));
        CHECK(!f.caller_holds(c.dst + c.bytes - 1) && !f.caller_holds(c.src + c.bytes - 1));
        const uint8_t *host = c.up ? c.src : c.dst;
        const Block &h = c.up ? f.hin : f.hout;
        const uint8_t *&end = c.up ? in_end : out_end;
        CHECK(h.holds(host) && host + c.bytes <= h.p + h.n);
        CHECK((host - h.p) % 16 == 0);
        CHECK(host >= end);                           // past every earlier slot
        end = host + c.bytes;
    }
    CHECK(f.dev.queued.size() == (size_t)((la != 0) + (lb != 0) + (lx != 0) + (ly != 0)));
    CHECK(f.outputs_untouched());
    f.dev.run();                                      // the device finishing does not reach the caller
    CHECK(f.outputs_untouched());
    CHECK(hc.finish() == MTCP_GPU_OK);
    CHECK(f.outputs_correct() && f.inputs_arrived());
    CHECK(f.s.npend == 0 && !f.dev.abandoned);
}

// up2 / down2: a pair adjacent on the device travels in one copy when bounded (up2: if its slots are adjacent)
void pairs(uint64_t la, uint64_t lb, uint64_t lx, uint64_t ly, bool bound) {
    Block a(la, 0), b(lb, 0), x(lx, kSentinel), y(ly, kSentinel), din(la + lb, 0), dout(lx + ly, 0);
    Block hin(lb ? pad(la) + lb : la, kPinned), hout(lx + ly, kPinned);
    a.set_pattern(1);
    b.set_pattern(2);
    dout.set_pattern(5);
    Stage s;
    s.h_in = hin.p, s.h_in_cap = hin.n, s.h_out = hout.p, s.h_out_cap = hout.n;
    FakeDevice dev;
    Call hc(s, Deadline(bound ? 1000000 : 0), {&dev});
    hc.up2(din.p, a.p, la, b.p, lb);
    hc.down2(x.p, dout.p, lx, y.p, ly);
    if (bound) {
        // inputs whose slots are adjacent (la a multiple of 16) go up in one copy
        CHECK(dev.queued.size() == (size_t)((la % 16 ? (la != 0) + (lb != 0) : la + lb != 0) + (lx + ly != 0)));
        for (const Copy &c : dev.queued)
            CHECK(!a.holds(c.src) && !b.holds(c.src) && !x.holds(c.dst) && !y.holds(c.dst));
    } else {
        CHECK(dev.queued.size() == (size_t)((la != 0) + (lb != 0) + (lx != 0) + (ly != 0)));
        CHECK(hin.all(kPinned) && hout.all(kPinned));
    }
    CHECK(x.all(kSentinel) && y.all(kSentinel));
    CHECK(hc.finish() == MTCP_GPU_OK);
    CHECK((!la || memcmp(din.p, a.p, la) == 0) && (!lb || memcmp(din.p + la, b.p, lb) == 0));
    CHECK((!lx || memcmp(x.p, dout.p, lx) == 0) && (!ly || memcmp(y.p, dout.p + lx, ly) == 0));
}

// 3. bounded, the drain times out: the late copies land in the bounce buffers only
void timed_out(uint64_t la, uint64_t lb, uint64_t lx, uint64_t ly) {
    Fixture f(la, lb, lx, ly);
    f.dev.stalled = true;
    Call hc(f.s, Deadline(1000000), {&f.dev});
    up_and_down(hc, f, false);
    CHECK(hc.finish() == MTCP_GPU_ETIMEDOUT);
    CHECK(f.dev.abandoned && f.s.npend == 0);
    CHECK(f.outputs_untouched());
    f.dev.run();                                      // what a stalled device does later
    CHECK(f.dev.ran == f.dev.queued.size());
    CHECK(f.outputs_untouched());
    f.dev.stalled = false;
    CHECK(hc.finish() == MTCP_GPU_ETIMEDOUT);         // no further wait, nothing copied
    CHECK(f.dev.drains == 1 && f.outputs_untouched());
}

// 4. the second of three copies fails to queue
void enqueue_fails(uint64_t la, uint64_t lb, uint64_t lx, bool bound) {
    Fixture f(la, lb, lx, 0);
    f.dev.fail_at = 1;
    Call hc(f.s, Deadline(bound ? 1000000 : 0), {&f.dev});
    hc.up(f.da.p, f.a.p, la);
    hc.up(f.db.p, f.b.p, lb);
    CHECK(!hc.ok());
    hc.down(f.x.p, f.dx.p, lx);
    CHECK(f.dev.queued.size() == 1 && f.dev.calls == 2);      // the third was never tried
    CHECK(hc.finish() == MTCP_GPU_EIO);
    CHECK(f.dev.drains == 1 && f.dev.ran == 1);               // the first copy was still drained
    CHECK(f.outputs_untouched() && f.s.npend == 0 && !f.dev.abandoned);
}

// 5. a slot may fill its buffer exactly; one byte more is refused and never written
void capacity() {
    for (uint64_t len : {1, 15, 16, 17, 33}) {
        for (int over = 0; over < 2; ++over) {
            for (int kind = 0; kind < 4; ++kind) {    // in, streamed in, down, down_pinned
                ++cur->cases;
                const uint64_t need = kind == 1 ? pad(len) : len;
                // 16 B in front: the slot under test is the buffer's second one
                Block hin(16 + need - over, kPinned), hout(16 + need - over, kPinned);
                Block src(len, 7), dst(len, kSentinel), d(len, 9), d16(16, 9), h16(16, 7);
                Stage s;
                s.h_in = hin.p, s.h_in_cap = hin.n, s.h_out = hout.p, s.h_out_cap = hout.n;
                FakeDevice dev;
                Call hc(s, Deadline(1000000), {&dev});
                hc.up(d16.p, h16.p, 16);
                hc.down(h16.p, d16.p, 16);
                CHECK(hc.ok() && dev.queued.size() == 2);
                if (kind == 0) hc.up(d.p, src.p, len);
                if (kind == 1) hc.up(d.p, src.p, len, true);
                if (kind == 2) hc.down(dst.p, d.p, len);
                const uint8_t *pin = kind == 3 ? hc.down_pinned(d.p, len) : nullptr;
                if (over) {
                    CHECK(!hc.ok() && dev.queued.size() == 2 && pin == nullptr && s.npend == 1);
                    CHECK(memcmp(hin.p, h16.p, 16) == 0);
                    for (uint64_t i = 16; i < hin.n; ++i) CHECK(hin.p[i] == kPinned);
                    CHECK(hout.all(kPinned));
                    CHECK(hc.finish() == MTCP_GPU_EIO && dev.drains == 1 && dst.all(kSentinel));
                } else {
                    CHECK(hc.ok() && dev.queued.size() == 3);
                    CHECK(hc.finish() == MTCP_GPU_OK);
                    if (kind < 2) CHECK(d.all(7));
                    if (kind == 2) CHECK(dst.all(9));
                    if (kind == 3) CHECK(pin == hout.p + 16 && memcmp(pin, d.p, len) == 0);
                }
            }
        }
    }
}

// 6. two rounds: each finish() copies out its own round only
void two_rounds(uint64_t lx, uint64_t ly, bool bound) {
    Fixture f(0, 0, lx, ly);
    Call hc(f.s, Deadline(bound ? 1000000 : 0), {&f.dev});
    hc.down(f.x.p, f.dx.p, lx);
    CHECK(hc.finish() == MTCP_GPU_OK && f.x.pattern(3) && f.y.all(kSentinel));
    if (lx) memset(f.x.p, kSentinel, lx);             // a second copy-out of round one would show
    f.dx.set_pattern(6);
    hc.down(f.y.p, f.dy.p, ly);
    if (bound && ly) CHECK(f.dev.queued.back().dst == f.hout.p);   // the slots started over
    CHECK(hc.finish() == MTCP_GPU_OK && f.y.pattern(4) && f.x.all(kSentinel));
    CHECK(f.dev.queued.size() == (size_t)((lx != 0) + (ly != 0)) && f.dev.drains == 2);
}

// 7. the stage's pending list as the rx pipeline uses it: a batch's records and option records
void pending_list(uint64_t lr, uint64_t lo) {
    Block rec(lr, kSentinel), opt(lo, kSentinel), hrec(lr, 0), hopt(lo, 0);
    hrec.set_pattern(8);
    hopt.set_pattern(9);
    Stage s;
    CHECK(stage_pend(s, rec.p, hrec.p, lr) && stage_pend(s, opt.p, hopt.p, lo) && s.npend == 2);
    CHECK(!stage_pend(s, rec.p, hopt.p, lo) && s.npend == 2);         // full: refused
    CHECK(rec.all(kSentinel) && opt.all(kSentinel));
    stage_copy_out(s);
    CHECK(s.npend == 0 && rec.pattern(8) && opt.pattern(9));
    if (lr) memset(rec.p, kSentinel, lr);
    stage_copy_out(s);                                                // cleared: nothing twice
    CHECK(rec.all(kSentinel));
    CHECK(stage_pend(s, rec.p, hrec.p, lr) && stage_pend(s, opt.p, hopt.p, lo));
    stage_drop(s);
    CHECK(s.npend == 0);
    stage_copy_out(s);
    CHECK(rec.all(kSentinel) && opt.pattern(9));
}

}  // namespace

int main() {
    Section sec[] = {{"unbounded"}, {"bounded"}, {"pairs"}, {"timed_out"}, {"enqueue_fails"},
                     {"capacity"}, {"two_rounds"}, {"pending_list"}};
    for (uint64_t la : kLens)
        for (uint64_t lb : kLens)
            for (uint64_t lx : kLens)
                for (uint64_t ly : kLens) {
                    cur = &sec[0], ++cur->cases, unbounded(la, lb, lx, ly);
                    cur = &sec[1], ++cur->cases, bounded(la, lb, lx, ly);
                    cur = &sec[2], cur->cases += 2, pairs(la, lb, lx, ly, false), pairs(la, lb, lx, ly, true);
                    cur = &sec[3], ++cur->cases, timed_out(la, lb, lx, ly);
                }
    cur = &sec[4];
    for (uint64_t la : {1, 15, 16, 17})               // three copies: none of them empty
        for (uint64_t lb : {1, 15, 16, 17})
            for (uint64_t lx : {1, 15, 16, 17})
                cur->cases += 2, enqueue_fails(la, lb, lx, false), enqueue_fails(la, lb, lx, true);
    cur = &sec[5], capacity();
    for (uint64_t lx : kLens)
        for (uint64_t ly : kLens) {
            cur = &sec[6], cur->cases += 2, two_rounds(lx, ly, false), two_rounds(lx, ly, true);
            cur = &sec[7], ++cur->cases, pending_list(lx, ly);
        }
    printf("{");
    for (size_t i = 0; i < sizeof(sec) / sizeof(sec[0]); ++i)
        printf("%s\"%s\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}", i ? ", " : "", sec[i].name,
               sec[i].cases, sec[i].bad, sec[i].first_line);
    printf("}\n");
    return 0;
}
