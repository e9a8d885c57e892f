// buffers.h — the format of the three byte buffers a forward leaves (geom, binning, img), stated once: struct Layout (byte offsets and
// extents: api.hip compute_layout fills it), the table that says which buffer holds a field and what its elements are, and Buffers, the
// typed view the launchers take.  Pure host code, no HIP: the includer defines float4 and uint2 (common.h has HIP's;
// tests/buffers_host_main.cpp, which checks every convention below over fake bases, has stand-ins).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/das3r_raster.h"

namespace das3r {

struct Layout {
    das3r_raster_layout pub;
    // private scratch offsets
    size_t g_keyA, g_keyB, g_valA, g_valB, g_hist, g_totals, g_blocksums, g_count, g_off_by_gid, g_rect;   // g_rect: u32 per splat, binned tile rectangle x0 | x1 << 8 | y0 << 16 | y1 << 24 (0 = none)
    size_t b_keyA, b_keyB, b_valA, b_valB, b_hist, b_totals, b_gid_of, b_slot;
    size_t b_e2;     // u32[capacity]: ping-pong partner of b_slot for the emission slots travelling through the partition passes
    size_t b_ckpt;   // float4[(capacity / BUCKET + ntiles + 2) * 256]: per-pixel (T, C) at the bucket boundaries of long tile lists
    // ABI 16: what a forward with out_invdepth appends to the binning buffer (pub.binning_bytes .. d_bytes; a colour-only forward's layout is
    // unchanged).  d_ckpt: per-pixel (T, D, 0, 0) at the same bucket boundaries as b_ckpt (D = inverse depth so far) — the depth as the first
    // colour of a checkpoint; d_recs / d_dpix / d_bg / d_dz: written by das3r_raster_backward_depth (api.hip) for its depth pass.
    size_t d_ckpt, d_recs, d_dpix, d_bg, d_dz, d_bytes;
    // single-pass radix control words (sort_onesweep.hip): [global digit histograms][tickets][status granules], contiguous
    // so that one store loop / one memset zeroes them: geom side by preprocess_kernel, binning side by a memset before emit
    size_t g_ghist, g_ticket, g_status, g_scan_status, g_ctrl_bytes;
    int64_t capacity;  // instance capacity the binning buffer was laid out for
    size_t b_ghist, b_ticket, b_status, b_ctrl_bytes;
    size_t b_cursor;   // u32[256 * cursor_stride] inside the control words: the bin cursors of the cells plan (cell_sort.hip)
    int cursor_stride; // words between two cursors: CURSOR_STRIDE (a 128-byte line each) from 2^20 instances on, 1 below (few workgroups; 1 KB to zero, not 32)
    int tiles_x, tiles_y, ntiles, tbits, tile_passes;
    int chunksP, chunksI;
    // segmented binning path (segkey.h): the partition key is (tile id << dbits | depth bucket), kbits = tbits + dbits wide, in the
    // SAME number of passes the tile ids alone need (the backward pass lays the buffers out without knowing the path).  dbits = 0
    // everywhere else.  g_dhist: u32[256] depth histogram of the forward
    int dbits, kbits, kshift;   // kshift: the key's low bits hold the fraction of the depth map (segkey.h: min(16, 32 - kbits) bits), the
                                // partition's digits start above them
    int part_passes;            // passes of the instance partition: tile_passes, or one more when the segmented path wants more bucket bits
    size_t g_dhist;
    size_t g_shjac;   // f32[9][P] behind everything else of the geometry buffer: plane 3c + k = d(rgb_c)/d(dir_k) (preprocess.hip); 0 = none
    const uint32_t *dhist_ptr;  // round 6: where this forward's depth histogram really is (a library-owned slot: forward.hip dhist_slots); null = geom + g_dhist
    size_t i_order;   // img buffer, u32[ntiles]: the tiles longest list first (render_regions.hip tile_lpt_kernel; round 6)
};

// The format: every offset field of Layout, the buffer it points into and its element type.  PUB: a field of das3r_raster_layout
// (Layout::pub, what include/das3r_raster.h documents); OWN: a private one.  Buffers has one accessor per row, named as the field.
// (recs: the geometry buffer — Buffers::recs says when it is not.)
#define DAS3R_BUFFER_FIELDS(PUB, OWN)                                                                                              \
    PUB(depth_key, geom, uint32_t) PUB(xy, recs, float4) PUB(conic_opacity, recs, float4) PUB(rgbd, recs, float4)                  \
    PUB(clamped, geom, uint8_t) PUB(tiles_touched, geom, uint32_t) PUB(sorted_idx, geom, uint32_t) PUB(offsets, geom, uint32_t)    \
    PUB(point_list, binning, uint32_t)                                                                                             \
    PUB(final_T, img, float) PUB(n_contrib, img, uint32_t) PUB(ranges, img, uint2)                                                 \
    OWN(g_keyA, geom, uint32_t) OWN(g_keyB, geom, uint32_t) OWN(g_valA, geom, uint32_t) OWN(g_valB, geom, uint32_t)                \
    OWN(g_hist, geom, uint32_t) OWN(g_totals, geom, uint32_t) OWN(g_blocksums, geom, uint32_t) OWN(g_count, geom, uint32_t)        \
    OWN(g_off_by_gid, geom, uint32_t) OWN(g_rect, geom, uint32_t) OWN(g_dhist, geom, uint32_t) OWN(g_shjac, geom, float)           \
    OWN(g_ghist, geom, uint32_t) OWN(g_ticket, geom, uint32_t) OWN(g_status, geom, unsigned long long)                             \
    OWN(g_scan_status, geom, unsigned long long)                                                                                   \
    OWN(b_keyA, binning, uint32_t) OWN(b_keyB, binning, uint32_t) OWN(b_valA, binning, uint32_t) OWN(b_valB, binning, uint32_t)    \
    OWN(b_hist, binning, uint32_t) OWN(b_totals, binning, uint32_t) OWN(b_gid_of, binning, uint32_t) OWN(b_slot, binning, uint32_t) \
    OWN(b_e2, binning, uint32_t) OWN(b_ckpt, binning, float4)                                                                      \
    OWN(b_ghist, binning, uint32_t) OWN(b_ticket, binning, uint32_t) OWN(b_cursor, binning, uint32_t)                              \
    OWN(b_status, binning, unsigned long long)                                                                                     \
    OWN(d_ckpt, binning, float4) OWN(d_recs, binning, float4) OWN(d_dpix, binning, float) OWN(d_bg, binning, float)                \
    OWN(d_dz, binning, float)                                                                                                      \
    OWN(i_order, img, uint32_t)

// a run of 32-bit control words that one memset / one store loop zeroes ({null, 0}: none)
struct WordRange {
    uint32_t *begin;
    size_t bytes;
    uint32_t words() const { return (uint32_t)(bytes / 4); }
};

// The three buffers and their layout.  The view OWNS its Layout (by value): das3r_raster_forward keeps one view per call and edits its L in
// place (dbits, kbits, kshift, part_passes, dhist_ptr; a new capacity when a too-small binning buffer is redone), the launchers take the view
// by reference, so every later launch sees those edits; the other entry points build one view from the saved state and pass it down.
// An accessor computes its pointer when it is called: one into a buffer that does not exist yet must not be.
struct Buffers {
    char *geom, *binning, *img;
    char *recs;   // the buffer that holds the splat records (xy, conic_opacity, rgbd): geom, except in the view depth_pass() returns
    Layout L;

#define DAS3R_PUB_ACCESSOR(field, buf, T) \
    T *field() const { return reinterpret_cast<T *>(buf + L.pub.field); }
#define DAS3R_OWN_ACCESSOR(field, buf, T) \
    T *field() const { return reinterpret_cast<T *>(buf + L.field); }
    DAS3R_BUFFER_FIELDS(DAS3R_PUB_ACCESSOR, DAS3R_OWN_ACCESSOR)
#undef DAS3R_PUB_ACCESSOR
#undef DAS3R_OWN_ACCESSOR

    // The 64 words at g_ticket, inside the zeroed geom-side control words: [0 .. 3] the tickets of the four depth-sort passes
    // (sort_onesweep.hip; b_ticket + p: those of the partition passes), [8] the binning self-check word, [16] the scan's ticket (scan_emit.hip).
    uint32_t *err_word() const { return g_ticket() + 8; }
    uint32_t *scan_ticket() const { return g_ticket() + 16; }
    // where this forward's depth histogram really is: a library-owned slot (forward.hip dhist_slots), or the geometry buffer's own
    const uint32_t *dhist() const { return L.dhist_ptr ? L.dhist_ptr : g_dhist(); }
    // the binned tile rectangles pack a coordinate into eight bits: absent (the emission bins again) past 255 tiles per axis
    const uint32_t *rect32() const { return (L.tiles_x <= 255 && L.tiles_y <= 255) ? g_rect() : nullptr; }
    // the SH colour's Jacobian planes; null when the layout has none (g_shjac is 0: the planes are never first in the buffer)
    float *shjac() const { return L.g_shjac ? g_shjac() : nullptr; }
    // the ping-pong partner of point_list: the passes alternate b_valA / b_valB so that the LAST one writes the buffer the layout calls
    // point_list, whatever their number (the backward pass lays the buffers out from tile_passes alone)
    uint32_t *point_list_partner() const { return L.pub.point_list == L.b_valA ? b_valB() : b_valA(); }
    // the control words of either side ([digit histograms][tickets][status granules], contiguous): geom's are zeroed by preprocess_kernel
    // (a memset when the binning is redone), binning's by preprocess_kernel, the last depth-sort pass or a memset before the emission
    WordRange g_ctrl() const { return {g_ghist(), L.g_ctrl_bytes}; }
    WordRange b_ctrl() const { return {b_ghist(), L.b_ctrl_bytes}; }
    // The depth pass of das3r_raster_backward_depth (api.hip backward_body) runs the compositing backward a second time over the binning
    // buffer's depth part: the splat records (xy, conic, (1/z, 0, 0, z)) depth_pass_inputs_kernel wrote at d_recs and the depth checkpoints
    // stand in for the geometry buffer's records and the colour checkpoints, and the background is the zero at d_bg.
    Buffers depth_pass(das3r_raster_args *ad) const {
        Buffers d = *this;
        d.recs = binning;
        d.L.pub.xy = L.d_recs;
        d.L.pub.conic_opacity = L.d_recs + 16;
        d.L.pub.rgbd = L.d_recs + 32;
        d.L.b_ckpt = L.d_ckpt;
        ad->bg = d_bg();
        return d;
    }
};

}  // namespace das3r
