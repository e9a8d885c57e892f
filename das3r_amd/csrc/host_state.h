// host_state.h — what the library remembers between calls, per host thread, and what api.hip and forward.hip need of each other.
#pragma once
#include "common.h"
#include "mailbox.h"

namespace das3r {

constexpr int MAX_DEVICES = 64;
// Everything the library remembers between calls, per host thread and per device (a thread that renders on two GPUs gets two
// of these; nothing is shared between threads: any number of them may render concurrently, each on its own stream).
struct PerDevice {
    Mailbox mb;
    CheckSlots checks;                              // self-check words not examined yet (mailbox.h)
    unsigned long long *arrive_ring = nullptr;      // self re-arming arrival words of the preprocess kernel's count reduction
    Verdict verdict;                                // what the last forward of the current shape (P, W, H) taught us (path_policy.h)
    Resume resume;                                  // das3r_raster_learning(set): handed to the next shape this thread meets
    char *emit_ring = nullptr;                      // control words of the emission fused into the preprocess kernel
    EmitRingState emit;
};
// forward.hip: this thread's state on the current device (created, with its mailbox, at the first call)
int per_device(PerDevice **out);
// api.hip (grid_is_resident): a second rendering thread on the device switches the ticket-free short cut off
void register_rendering_thread(int dev);
// forward.hip: what every entry that takes (args, in) asks of them
int validate(const das3r_raster_args *a, const das3r_raster_in *in);
// forward.hip: a self-check word {flags, tag} -> 1 not there, DAS3R_OK, or DAS3R_ERR_HIP (reported once); das3r_raster_check waits for it
int examine_check_slot(volatile uint32_t *slot, uint32_t tag, bool wait, hipStream_t s);
bool split_colour_rule(bool has_sh, int sh_degree, int P, int binning_path, bool no_backward, int forced);

}  // namespace das3r
