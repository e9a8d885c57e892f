// mailbox.h — the host side of the host <-> device hand-off protocol of a forward: the words of the pinned mailbox, the tags that name
// a hand-off, the examination of a binning self-check word, the per-thread bookkeeping of the sixteen check slots and the "zero it again"
// rule of the emission ring.  Pure host arithmetic over a block of words: no HIP, no switches(), no error reporting — forward.hip owns the
// mailbox's memory, does the waiting (await_tag: a bounded spin, hipStreamQuery, at last hipStreamSynchronize; handed in here as a
// callable), and turns a CheckResult into statistics, the verbose line and the error string.  Compiles alone with a host compiler
// (tests/mailbox_host_main.cpp drives it over plain memory).
#pragma once
#include <stdint.h>

namespace das3r {

// Host mailbox: a pinned, device-visible block per host thread and device.  The scan kernel stores {count, flags} and then the
// tag of the call (system-scope release) into words 0..2; word 10 is raised by a compositing kernel that met a tile list too
// long for its LDS sort; the last binning kernel of a forward stores {self-check word, tag} into one of CHECK_SLOTS two-word
// slots from word 16 on (slot = tag % CHECK_SLOTS).  The host polls the tags — no D2H copy kernel, no event, no parked thread
// (hipEventSynchronize's wake-up alone cost ~100 us per forward, a third of a 100 k-splat step).
struct Mailbox {
    volatile uint32_t *host = nullptr;
    uint32_t *dev = nullptr;
    uint32_t seq = 0;
};
// the words the host reads by index (the kernels are handed pointers: dev + MB_COUNT {count, flags, tag}, dev + MB_TOO_LONG {too long,
// want bits}, dev + MB_LONGEST {longest, tag, crowding})
enum MailboxWord : uint32_t {
    MB_COUNT = 0,       // num_rendered of the forward whose tag is in MB_COUNT_TAG
    MB_COUNT_TAG = 2,
    MB_TOO_LONG = 10,   // != 0: a forward of the shape with that generation number met a list too long for LDS (path_policy.h)
    MB_WANT_BITS = 11,  // != 0: the segmented path of that generation sorted a segment long enough to want more bucket bits
    MB_FILTERED = 12,   // the tag of a forward whose preprocess kernel culled a point
    MB_LONGEST = 13,    // list_skew_kernel: the longest tile list of the forward whose tag is in MB_SKEW_TAG
    MB_SKEW_TAG = 14,
    MB_CROWD16 = 15,    // ... and of 64 consecutive list entries, those in the tile's fullest quadrant, x 16
};
constexpr uint32_t CHECK_SLOTS = 16, CHECK_WORD0 = 16, MAILBOX_BYTES = 4 * (CHECK_WORD0 + 2 * CHECK_SLOTS);
// the tag of the next hand-off through the mailbox (never 0: an empty word names nobody)
static inline uint32_t next_tag(Mailbox *mb) { return ++mb->seq ? mb->seq : ++mb->seq; }
// the check slot the forward with that tag delivers its self-check word to, and the slot's first word {flags, tag} in the mailbox
static inline uint32_t check_slot_of(uint32_t tag) { return tag % CHECK_SLOTS; }
static inline uint32_t check_word_index(uint32_t slot) { return CHECK_WORD0 + 2 * slot; }

// The self-check word a forward's last binning kernel left in `slot` = {flags, tag}: bit 1 look-back timeout, 2 index out of range ->
// write suppressed, 8 counts do not add up to the histogram; 16 = a stalled look-back was rescued (granule.h: informational); bit 31 is the
// host's own: this forward's failure has been reported already (by the backward pass / das3r_raster_check).
constexpr uint32_t CHECK_RESCUED = 16u, CHECK_REPORTED_BIT = 0x80000000u;
enum CheckState { CHECK_NOT_THERE, CHECK_FINE, CHECK_REPORTED, CHECK_FAILED };
struct CheckResult {
    CheckState state;
    uint32_t flags;   // CHECK_FAILED: the failure bits (without the informational one)
    uint32_t stats;   // bit i set: count one more in statistic i (1 words examined, 2 rescued look-back polls, 3 failed self-checks)
    bool rescued;     // the informational bit was set (the verbose line)
    int error;        // what the wait callable returned when it failed (the state is then CHECK_NOT_THERE), else 0
};
// wait: spin (bounded) until the word of `tag` is there — await(word, tag, &seen) -> 0 or an error, *seen = what the word held at its last
// look.  CHECK_NOT_THERE: the slot does not hold `tag`'s word (not there yet, or — after CHECK_SLOTS later forwards, each of which
// examines the slot before reusing it — gone).  A failure is marked reported in the word itself: the thread that made the forward will not
// report it again at its next call.
template <class Await>
static inline CheckResult examine_check_word(volatile uint32_t *slot, uint32_t tag, bool wait, Await &&await) {
    CheckResult r = {CHECK_NOT_THERE, 0u, 0u, false, 0};
    uint32_t seen = __atomic_load_n(&slot[1], __ATOMIC_ACQUIRE);
    if (seen != tag && wait && (r.error = await(&slot[1], tag, &seen))) return r;
    if (seen != tag) return r;
    const uint32_t all_flags = slot[0];
    r.flags = all_flags & ~(CHECK_RESCUED | CHECK_REPORTED_BIT);
    if (all_flags & CHECK_REPORTED_BIT) { r.state = CHECK_REPORTED; return r; }
    r.rescued = (all_flags & CHECK_RESCUED) != 0;
    r.stats = 1u << 1 | (r.rescued ? 1u << 2 : 0u) | (r.flags ? 1u << 3 : 0u);
    r.state = r.flags ? CHECK_FAILED : CHECK_FINE;
    if (r.flags) slot[0] = all_flags | CHECK_REPORTED_BIT;
    return r;
}

// Per host thread and device, per check slot: the tag of the forward whose self-check word has not been examined yet (0: none).
// examine(slot, tag, wait) -> 1 when the slot does not hold the tag's word, 0 when the word was fine, < 0 an error (a failed self-check,
// reported once: the entry is forgotten either way).
struct CheckSlots {
    uint32_t pending[CHECK_SLOTS] = {};
    template <class Examine>
    int settle(uint32_t i, bool wait, Examine &&examine) {
        if (!pending[i]) return 0;
        const int r = examine(i, pending[i], wait);
        if (r == 1) return 0;   // not there yet: look again next time
        pending[i] = 0;
        return r;
    }
    // the look without waiting at the start of a forward, for callers that use neither das3r_raster_backward nor das3r_raster_check
    template <class Examine>
    int settle_all(Examine &&examine) {
        for (uint32_t i = 0; i < CHECK_SLOTS; i++)
            if (const int r = settle(i, false, examine)) return r;
        return 0;
    }
    // wait for the forward that used `tag`'s slot CHECK_SLOTS forwards ago, then the slot is `tag`'s; *slot = which
    template <class Examine>
    int claim(uint32_t tag, uint32_t *slot, Examine &&examine) {
        *slot = check_slot_of(tag);
        if (const int r = settle(*slot, true, examine)) return r;
        pending[*slot] = tag;
        return 0;
    }
};

// The emission ring (control words of the emission fused into the preprocess kernel: one slot per forward, zero at rest, versioned by the
// forward's tag) is zeroed again on first use, after an aborted forward (dirty: taken and never re-armed) and when the tags wrapped around.
struct EmitRingState {
    bool dirty = true;   // (nobody has zeroed it yet)
    uint32_t last_tag = 0;
    bool wants_zeroing(uint32_t tag) const { return dirty || tag < last_tag; }
    void zeroed() { dirty = false; }
    void taken_by(uint32_t tag) { last_tag = tag; dirty = true; }   // until the last binning kernel of that forward is enqueued (it re-arms the slot)
    void rearmed() { dirty = false; }
};

}  // namespace das3r
