// preprocess_plan.h -- the host side of siggan_preprocess_u8's geometry: what a (n, 4) table {offset, height, width,
// min_pixels} must satisfy, and where each scan's scratch lies in the workspace.  No HIP in it: it compiles with -x c++,
// which is how preprocess_plan_check.cpp holds it to what the kernels need (every scratch range inside the workspace and
// disjoint from every other).
//
// A scan's scratch is placed by its pool offset and its index alone, so no prefix over the batch is needed on the device:
// offsets ascend with the index (refused otherwise), so floor(offset / d) + slack * index ascends at least as fast as the
// ranges grow.  For the row masks (one 64-bit word per 64 columns of a row) h * ceil(w / 64) <= floor(h * w / 64) + 1 + 63 * h / 64
// <= floor(h * w / 64) + 1009; for the run slots (one per two columns of a row) h * ceil(w / 2) <= floor(h * w / 2) + 513.
// Both fit the slack of 1024 per scan.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int PP_MIN_SIDE = 16, PP_MAX_SIDE = 1024, PP_MAX_MARGIN = 64, PP_MAX_BATCH = 65536;
constexpr int PP_TILE = 64;                      // k_pp_denoise's output tile
constexpr int PP_MAX_TILES = (PP_MAX_SIDE / PP_TILE) * (PP_MAX_SIDE / PP_TILE);   // WHITE partials per scan
constexpr int PP_SLACK = 1024;                   // per-scan slack of the mask and slot ranges (see above)
constexpr int PP_BOX_INTS = 8;                   // k_pp_label's per-scan result: components, kept, x0, y0, x1, y1, overflow, spare

// Where the parts of the workspace begin, in bytes from its (8-byte aligned) start, and its size.
struct PpLayout {
    size_t pool, masks, lab, area, partials, boxes, bytes;
    int64_t mask_words, slots;                   // extents of masks (uint64) and of lab / area (int32 each)
};

inline PpLayout pp_layout(int64_t total_pixels, int64_t n) {
    PpLayout L;
    L.mask_words = (total_pixels >> 6) + (int64_t)PP_SLACK * n;
    L.slots = (total_pixels >> 1) + (int64_t)PP_SLACK * n;
    L.pool = 0;
    L.masks = ((size_t)total_pixels + 7) & ~(size_t)7;
    L.lab = L.masks + 8 * (size_t)L.mask_words;
    L.area = L.lab + 4 * (size_t)L.slots;
    L.partials = L.area + 4 * (size_t)L.slots;
    L.boxes = L.partials + 4 * (size_t)PP_MAX_TILES * (size_t)n;
    L.bytes = L.boxes + 4 * (size_t)PP_BOX_INTS * (size_t)n;
    return L;
}

// First mask word / first run slot of scan i at pool offset `offset` (the kernels compute the same two expressions).
inline int64_t pp_mask_base(int64_t offset, int64_t i) { return (offset >> 6) + (int64_t)PP_SLACK * i; }
inline int64_t pp_slot_base(int64_t offset, int64_t i) { return (offset >> 1) + (int64_t)PP_SLACK * i; }
inline int pp_mask_words(int h, int w) { return h * ((w + 63) >> 6); }
inline int pp_slots(int h, int w) { return h * ((w + 1) >> 1); }
inline int pp_tiles(int h, int w) { return ((h + PP_TILE - 1) / PP_TILE) * ((w + PP_TILE - 1) / PP_TILE); }

// What is wrong with the table, as a code and the scan it is about; PP_GEOM_OK when nothing is.  max_tiles: the largest
// tile count of a scan, which sizes k_pp_denoise's grid.
enum PpGeomError { PP_GEOM_OK, PP_GEOM_HEIGHT, PP_GEOM_WIDTH, PP_GEOM_MIN_PIXELS, PP_GEOM_OFFSET_NEGATIVE, PP_GEOM_OFFSET_ORDER,
                   PP_GEOM_OFFSET_PAST_END };

inline PpGeomError pp_check_geometry(const int64_t* geom, int64_t n, int64_t total_pixels, int64_t* at, int* max_tiles) {
    int64_t end = 0;                             // one past the last byte of the scans so far
    int tiles = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t off = geom[4 * i], h = geom[4 * i + 1], w = geom[4 * i + 2], mp = geom[4 * i + 3];
        *at = i;
        if (h < PP_MIN_SIDE || h > PP_MAX_SIDE) return PP_GEOM_HEIGHT;
        if (w < PP_MIN_SIDE || w > PP_MAX_SIDE) return PP_GEOM_WIDTH;
        if (mp < 1) return PP_GEOM_MIN_PIXELS;
        if (off < 0) return PP_GEOM_OFFSET_NEGATIVE;
        if (off < end) return PP_GEOM_OFFSET_ORDER;
        if (off > total_pixels - h * w) return PP_GEOM_OFFSET_PAST_END;
        end = off + h * w;
        const int t = pp_tiles((int)h, (int)w);
        tiles = t > tiles ? t : tiles;
    }
    *max_tiles = tiles;
    return PP_GEOM_OK;
}
