// The host <-> device hand-off protocol of a forward (das3r_amd/csrc/mailbox.h) over plain memory: tags, slot arithmetic, the examination of a
// self-check word, the per-thread bookkeeping of the check slots and the emission ring's "zero it again" rule.  Includes only mailbox.h;
// built with -fsanitize=address,undefined and run by tests/test_mailbox_host.py.  Exits non-zero on a wrong answer.
#include <cstdio>
#include <vector>

#include "../das3r_amd/csrc/mailbox.h"

using namespace das3r;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "mailbox_host: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static uint32_t g_stats[4];
static void bump(const CheckResult &r) {
    for (int i = 0; i < 4; i++) g_stats[i] += r.stats >> i & 1u;
}
static bool stats_are(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
    return g_stats[0] == s0 && g_stats[1] == s1 && g_stats[2] == s2 && g_stats[3] == s3;
}
// a wait that must not happen, and one that is recorded and delivers nothing
static int no_wait(volatile uint32_t *, uint32_t, uint32_t *) { return -99; }
struct Waited { volatile uint32_t *word; uint32_t tag; };
static std::vector<Waited> g_waited;
static int recorded_wait(volatile uint32_t *word, uint32_t tag, uint32_t *seen) {
    g_waited.push_back({word, tag});
    *seen = *word;
    return 0;
}

int main() {
    // tag wrap: never 0
    Mailbox mb;
    mb.seq = 0xFFFFFFFEu;
    CHECK(next_tag(&mb) == 0xFFFFFFFFu);
    CHECK(next_tag(&mb) == 1u);
    CHECK(next_tag(&mb) == 2u);
    // indices
    static_assert(MAILBOX_BYTES == 192, "16 words + 16 slots of two");
    static_assert(CHECK_SLOTS == 16 && CHECK_WORD0 == 16, "");
    static_assert(MB_COUNT == 0 && MB_COUNT_TAG == 2 && MB_TOO_LONG == 10 && MB_WANT_BITS == 11 && MB_FILTERED == 12 && MB_LONGEST == 13 && MB_SKEW_TAG == 14 && MB_CROWD16 == 15, "");
    CHECK(check_slot_of(1) == 1 && check_slot_of(16) == 0 && check_slot_of(35) == 3 && check_slot_of(0xFFFFFFFFu) == 15);
    CHECK(check_word_index(0) == 16 && check_word_index(3) == 22 && check_word_index(15) == 46);
    CHECK(4 * (check_word_index(CHECK_SLOTS - 1) + 2) == MAILBOX_BYTES);

    uint32_t words[MAILBOX_BYTES / 4] = {};
    volatile uint32_t *slot = words + check_word_index(check_slot_of(35));
    // not there: the slot holds another tag's word
    slot[0] = 1u;
    slot[1] = 19u;
    CheckResult r = examine_check_word(slot, 35u, false, no_wait);
    bump(r);
    CHECK(r.state == CHECK_NOT_THERE && r.error == 0 && r.stats == 0 && stats_are(0, 0, 0, 0) && slot[0] == 1u);
    // ... and a wait that fails is handed back
    r = examine_check_word(slot, 35u, true, no_wait);
    CHECK(r.state == CHECK_NOT_THERE && r.error == -99 && r.stats == 0);
    // fine
    slot[0] = 0u;
    slot[1] = 35u;
    r = examine_check_word(slot, 35u, true, no_wait);   // (there already: nobody waits)
    bump(r);
    CHECK(r.state == CHECK_FINE && r.flags == 0 && !r.rescued && stats_are(0, 1, 0, 0) && slot[0] == 0u);
    // a rescued look-back poll is fine
    slot[0] = 16u;
    r = examine_check_word(slot, 35u, false, no_wait);
    bump(r);
    CHECK(r.state == CHECK_FINE && r.flags == 0 && r.rescued && stats_are(0, 2, 1, 0) && slot[0] == 16u);
    // a failure: its flags without the informational bit, reported once
    slot[0] = 1u | 16u;
    r = examine_check_word(slot, 35u, false, no_wait);
    bump(r);
    CHECK(r.state == CHECK_FAILED && r.flags == 0x1u && r.rescued && stats_are(0, 3, 2, 1));
    CHECK(slot[0] == (1u | 16u | 0x80000000u) && slot[1] == 35u);
    r = examine_check_word(slot, 35u, false, no_wait);
    bump(r);
    CHECK(r.state == CHECK_REPORTED && r.stats == 0 && !r.rescued && r.error == 0 && stats_are(0, 3, 2, 1) && slot[0] == (1u | 16u | 0x80000000u));

    // slot reuse: seventeen claims in a row, no word delivered
    for (auto &w : words) w = 0;
    CheckSlots slots;
    Mailbox m2;
    auto examine = [&](uint32_t i, uint32_t tag, bool wait) {
        const CheckResult c = examine_check_word(words + check_word_index(i), tag, wait, recorded_wait);
        return c.error ? c.error : c.state == CHECK_NOT_THERE ? 1 : c.state == CHECK_FAILED ? -3 : 0;
    };
    uint32_t first_tag = 0, first_slot = 0;
    for (int k = 0; k < 17; k++) {
        CHECK(slots.settle_all(examine) == 0 && g_waited.empty());   // the look at the start of a forward never waits
        const uint32_t tag = next_tag(&m2);
        uint32_t s = 99;
        if (k < 16) {
            CHECK(slots.claim(tag, &s, examine) == 0 && g_waited.empty());
            CHECK(s == check_slot_of(tag) && slots.pending[s] == tag);
            if (k == 0) { first_tag = tag; first_slot = s; }
        } else {
            CHECK(check_slot_of(tag) == first_slot && slots.pending[first_slot] == first_tag);
            CHECK(slots.claim(tag, &s, examine) == 0);
            CHECK(g_waited.size() == 1 && g_waited[0].tag == first_tag && g_waited[0].word == words + check_word_index(first_slot) + 1);
            CHECK(s == first_slot && slots.pending[s] == tag);
        }
    }
    // a delivered failure is handed back by the look, once, and the entry forgotten
    const uint32_t t2 = slots.pending[2];
    words[check_word_index(2)] = 8u;
    words[check_word_index(2) + 1] = t2;
    CHECK(t2 != 0 && slots.settle_all(examine) == -3 && slots.pending[2] == 0 && slots.settle_all(examine) == 0);

    // emission ring
    EmitRingState ring;
    CHECK(ring.wants_zeroing(5));        // first use
    ring.zeroed();
    ring.taken_by(5);
    CHECK(ring.wants_zeroing(6));        // taken and never re-armed: an aborted forward
    ring.rearmed();
    CHECK(!ring.wants_zeroing(6) && !ring.wants_zeroing(5));
    ring.taken_by(6);
    ring.rearmed();
    CHECK(ring.wants_zeroing(1));        // the tags went backwards
    ring.zeroed();
    ring.taken_by(1);
    ring.rearmed();
    CHECK(!ring.wants_zeroing(2));
    printf("mailbox_host: all checks passed\n");
    return 0;
}
