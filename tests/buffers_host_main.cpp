// The format of a forward's three buffers (das3r_amd/csrc/buffers.h) over fake bases and a hand-filled Layout: every table accessor lands
// in its buffer at its field's offset, and each convention that used to exist only as copies at the launch sites — the words inside
// g_ticket, the depth histogram's override, the rectangles' limit of 255 tiles, the absent Jacobian planes, the ping-pong partner of
// point_list, the control-word ranges, the depth pass's re-based view — is where the kernels' launchers expect it.  Includes only buffers.h;
// built with -fsanitize=address,undefined and run by tests/test_buffers_host.py.  Exits non-zero on a wrong answer.
#include <cstdio>
#include <cstring>
#include <type_traits>

struct float4 { float x, y, z, w; };
struct uint2 { unsigned x, y; };
#include "../das3r_amd/csrc/buffers.h"

using namespace das3r;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "buffers_host: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static char g_geom[1 << 15], g_binning[1 << 15], g_img[1 << 15];

// pairwise distinct offsets, 256 bytes apart (room for the + 16 / + 32 of the depth records and the ticket words), in table order
static Layout distinct_layout() {
    Layout L;
    memset(&L, 0, sizeof(L));
    size_t next = 256;
#define FILL_PUB(field, buf, T) L.pub.field = next, next += 256;
#define FILL_OWN(field, buf, T) L.field = next, next += 256;
    DAS3R_BUFFER_FIELDS(FILL_PUB, FILL_OWN)
#undef FILL_PUB
#undef FILL_OWN
    L.g_ctrl_bytes = 4 * 1000;
    L.b_ctrl_bytes = 4 * 2000;
    L.tiles_x = L.tiles_y = 8;
    L.tile_passes = 1;
    return L;
}

template <class T>
static bool at(const T *p, const char *base, size_t off) { return reinterpret_cast<const char *>(p) == base + off; }

// the four accessors the depth pass re-bases
static bool rebased(const char *field) {
    return !strcmp(field, "xy") || !strcmp(field, "conic_opacity") || !strcmp(field, "rgbd") || !strcmp(field, "b_ckpt");
}
// every table accessor of `v` in its buffer at L's offset (recs: the geometry buffer) — but for the re-based ones when `depth_view`
static int table_lands(const Buffers &v, const Layout &L, bool depth_view) {
    const char *geom = v.geom, *binning = v.binning, *img = v.img, *recs = v.geom;
    int n = 0;
#define LANDS_PUB(field, buf, T) if (!(depth_view && rebased(#field))) { CHECK(at(v.field(), buf, L.pub.field)); n++; }
#define LANDS_OWN(field, buf, T) if (!(depth_view && rebased(#field))) { CHECK(at(v.field(), buf, L.field)); n++; }
    DAS3R_BUFFER_FIELDS(LANDS_PUB, LANDS_OWN)
#undef LANDS_PUB
#undef LANDS_OWN
    CHECK(n == (depth_view ? 44 : 48));   // (every offset field of Layout has its row)
    (void)geom; (void)binning; (void)img; (void)recs;
    return 0;
}

int main() {
    const Layout L = distinct_layout();
    Buffers v = {g_geom, g_binning, g_img, g_geom, L};
    CHECK(sizeof(g_geom) > L.i_order + 256);   // (every offset is inside the fake buffers)

    // the table: each accessor in its buffer at its field's offset
    if (table_lands(v, L, false)) return 1;
    CHECK(v.recs == v.geom);
    // the element types the compositing kernels read
    static_assert(std::is_same<decltype(v.ranges()), uint2 *>::value, "ranges");
    static_assert(std::is_same<decltype(v.point_list()), uint32_t *>::value, "point_list");
    static_assert(std::is_same<decltype(v.xy()), float4 *>::value, "xy");
    static_assert(std::is_same<decltype(v.conic_opacity()), float4 *>::value, "conic_opacity");
    static_assert(std::is_same<decltype(v.rgbd()), float4 *>::value, "rgbd");
    static_assert(std::is_same<decltype(v.n_contrib()), uint32_t *>::value, "n_contrib");
    static_assert(std::is_same<decltype(v.final_T()), float *>::value, "final_T");
    static_assert(std::is_same<decltype(v.b_slot()), uint32_t *>::value, "b_slot");
    static_assert(std::is_same<decltype(v.b_ckpt()), float4 *>::value, "b_ckpt");
    static_assert(std::is_same<decltype(v.g_scan_status()), unsigned long long *>::value, "the granules are 64-bit");

    // the depth histogram: the geometry buffer's own unless the forward took a library-owned slot
    CHECK(v.dhist() == v.g_dhist() && at(v.dhist(), g_geom, L.g_dhist));
    uint32_t slot[256];
    v.L.dhist_ptr = slot;
    CHECK(v.dhist() == slot && at(v.g_dhist(), g_geom, L.g_dhist));
    v.L.dhist_ptr = nullptr;

    // the binned rectangles: up to 255 tiles per axis, either axis
    v.L.tiles_x = 255, v.L.tiles_y = 255;
    CHECK(v.rect32() == v.g_rect() && at(v.rect32(), g_geom, L.g_rect));
    v.L.tiles_x = 256, v.L.tiles_y = 1;
    CHECK(v.rect32() == nullptr);
    v.L.tiles_x = 1, v.L.tiles_y = 256;
    CHECK(v.rect32() == nullptr);
    v.L.tiles_x = L.tiles_x, v.L.tiles_y = L.tiles_y;

    // the Jacobian planes: absent when the layout has none
    CHECK(v.shjac() == v.g_shjac() && at(v.shjac(), g_geom, L.g_shjac));
    v.L.g_shjac = 0;
    CHECK(v.shjac() == nullptr);
    v.L.g_shjac = L.g_shjac;

    // the words inside g_ticket, and the binning side's tickets
    CHECK(at(v.err_word(), g_geom, L.g_ticket + 4 * 8));
    CHECK(at(v.scan_ticket(), g_geom, L.g_ticket + 4 * 16));
    CHECK(at(v.g_ticket(), g_geom, L.g_ticket) && at(v.b_ticket(), g_binning, L.b_ticket));

    // the ping-pong partner of point_list, as compute_layout sets point_list for either parity of tile_passes
    for (int passes = 1; passes <= 4; passes++) {
        v.L.tile_passes = passes;
        v.L.pub.point_list = (passes & 1) ? L.b_valB : L.b_valA;
        CHECK(v.point_list() == ((passes & 1) ? v.b_valB() : v.b_valA()));
        CHECK(v.point_list_partner() == ((passes & 1) ? v.b_valA() : v.b_valB()));
        CHECK(v.point_list_partner() != v.point_list());
    }
    v.L.tile_passes = L.tile_passes, v.L.pub.point_list = L.pub.point_list;

    // the control words of either side
    CHECK(at(v.g_ctrl().begin, g_geom, L.g_ghist) && v.g_ctrl().bytes == L.g_ctrl_bytes && v.g_ctrl().words() == 1000u);
    CHECK(at(v.b_ctrl().begin, g_binning, L.b_ghist) && v.b_ctrl().bytes == L.b_ctrl_bytes && v.b_ctrl().words() == 2000u);

    // the depth pass: records and checkpoints from the binning buffer's depth part, the background at d_bg, everything else as it was
    das3r_raster_args ad;
    memset(&ad, 0, sizeof(ad));
    const Buffers d = v.depth_pass(&ad);
    CHECK(at(d.xy(), g_binning, L.d_recs) && at(d.conic_opacity(), g_binning, L.d_recs + 16) && at(d.rgbd(), g_binning, L.d_recs + 32));
    CHECK(at(d.b_ckpt(), g_binning, L.d_ckpt) && d.b_ckpt() == v.d_ckpt());
    CHECK(ad.bg == v.d_bg() && at(ad.bg, g_binning, L.d_bg));
    CHECK(d.geom == g_geom && d.binning == g_binning && d.img == g_img);
    if (table_lands(d, L, true)) return 1;
    // ... and the view it was made from is untouched
    if (table_lands(v, L, false)) return 1;

    printf("all checks passed\n");
    return 0;
}
