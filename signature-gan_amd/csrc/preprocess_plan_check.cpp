// preprocess_plan_check.cpp -- a stand-alone host program (no device, not part of the library) that holds preprocess_plan.h
// to what the kernels of preprocess.hip need: a scan's row masks and run slots, placed by its pool offset and its index
// alone, lie inside the workspace and do not meet the next scan's, for every height and width in 16..1024 at offsets of
// every residue that matters and for seeded ragged batches with gaps; and pp_check_geometry refuses each kind of bad table
// at the right scan.  tests/test_preprocess_cpu.py builds it with the host compiler under AddressSanitizer and UBSan and
// runs it.  Prints "OK <cases>" and returns 0, or "FAIL ..." and 1.
#include <stdio.h>

#include <vector>

#include "preprocess_plan.h"

static int fail(const char* what, long long a, long long b, long long c) {
    printf("FAIL %s: %lld, %lld, %lld\n", what, a, b, c);
    return 1;
}

int main() {
    long cases = 0;
    // 1. one scan and its successor at the tightest spacing
    const int residues[] = {0, 1, 2, 31, 63, 64, 65, 127};
    for (int h = PP_MIN_SIDE; h <= PP_MAX_SIDE; ++h)
        for (int w = PP_MIN_SIDE; w <= PP_MAX_SIDE; ++w)
            for (int o : residues) {
                const int64_t next = (int64_t)o + (int64_t)h * w;
                if (pp_mask_base(o, 0) + pp_mask_words(h, w) > pp_mask_base(next, 1)) return fail("mask ranges meet", h, w, o);
                if (pp_slot_base(o, 0) + pp_slots(h, w) > pp_slot_base(next, 1)) return fail("slot ranges meet", h, w, o);
                const PpLayout L = pp_layout(next, 1);
                if (pp_mask_base(o, 0) + pp_mask_words(h, w) > L.mask_words) return fail("masks past the end", h, w, o);
                if (pp_slot_base(o, 0) + pp_slots(h, w) > L.slots) return fail("slots past the end", h, w, o);
                if (pp_tiles(h, w) < 1 || pp_tiles(h, w) > PP_MAX_TILES) return fail("tiles", h, w, pp_tiles(h, w));
                ++cases;
            }
    // 2. seeded ragged batches with gaps
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto rnd = [&state](int lo, int hi) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return lo + (int)((state >> 33) % (uint64_t)(hi - lo + 1));
    };
    for (int trial = 0; trial < 200; ++trial) {
        const int n = rnd(1, 40);
        std::vector<int64_t> geom(4 * (size_t)n);
        int64_t off = 0;
        int want_tiles = 0;
        for (int i = 0; i < n; ++i) {
            const int h = rnd(0, 3) ? rnd(PP_MIN_SIDE, 80) : rnd(PP_MIN_SIDE, PP_MAX_SIDE), w = rnd(0, 3) ? rnd(PP_MIN_SIDE, 80) : rnd(PP_MIN_SIDE, PP_MAX_SIDE);
            off += rnd(0, 2) ? 0 : rnd(1, 200);
            geom[4 * i] = off; geom[4 * i + 1] = h; geom[4 * i + 2] = w; geom[4 * i + 3] = rnd(1, 50);
            off += (int64_t)h * w;
            want_tiles = pp_tiles(h, w) > want_tiles ? pp_tiles(h, w) : want_tiles;
        }
        const int64_t total = off + rnd(0, 5);
        int64_t at = -1;
        int tiles = 0;
        if (pp_check_geometry(geom.data(), n, total, &at, &tiles) != PP_GEOM_OK || tiles != want_tiles) return fail("a sound table refused", trial, at, tiles);
        const PpLayout L = pp_layout(total, n);
        if (!(L.pool < L.masks && L.masks % 8 == 0 && L.masks >= (size_t)total && L.masks < L.lab && L.lab < L.area && L.area < L.partials &&
              L.partials < L.boxes && L.boxes < L.bytes && L.lab % 4 == 0))
            return fail("layout out of order", trial, (long long)L.masks, (long long)L.bytes);
        int64_t mask_end = 0, slot_end = 0;
        for (int i = 0; i < n; ++i, ++cases) {
            const int64_t o = geom[4 * i];
            const int h = (int)geom[4 * i + 1], w = (int)geom[4 * i + 2];
            if (pp_mask_base(o, i) < mask_end || pp_slot_base(o, i) < slot_end) return fail("ranges overlap", trial, i, o);
            mask_end = pp_mask_base(o, i) + pp_mask_words(h, w);
            slot_end = pp_slot_base(o, i) + pp_slots(h, w);
        }
        if (mask_end > L.mask_words || slot_end > L.slots) return fail("ranges past the end", trial, mask_end, slot_end);
        // 3. every kind of bad table, at a scan chosen by the trial
        const int k = rnd(0, n - 1);
        struct { int column; int64_t value; PpGeomError want; } bad[] = {
            {1, PP_MIN_SIDE - 1, PP_GEOM_HEIGHT}, {1, PP_MAX_SIDE + 1, PP_GEOM_HEIGHT}, {2, PP_MIN_SIDE - 1, PP_GEOM_WIDTH},
            {2, PP_MAX_SIDE + 1, PP_GEOM_WIDTH}, {3, 0, PP_GEOM_MIN_PIXELS}, {0, -1, PP_GEOM_OFFSET_NEGATIVE},
            {0, total, PP_GEOM_OFFSET_PAST_END}};
        for (const auto& b : bad) {
            std::vector<int64_t> g = geom;
            g[4 * (size_t)k + b.column] = b.value;
            const PpGeomError got = pp_check_geometry(g.data(), n, total, &at, &tiles);
            if (got != b.want || at != k) return fail("wrong refusal", trial, got, at);
            ++cases;
        }
        if (k > 0) {
            std::vector<int64_t> g = geom;
            g[4 * (size_t)k] = geom[4 * (size_t)(k - 1)] + geom[4 * (size_t)(k - 1) + 1] * geom[4 * (size_t)(k - 1) + 2] - 1;   // one byte into the scan before
            if (pp_check_geometry(g.data(), n, total, &at, &tiles) != PP_GEOM_OFFSET_ORDER || at != k) return fail("overlap not refused", trial, k, at);
            ++cases;
        }
        if (pp_check_geometry(geom.data(), n, geom[4 * (size_t)(n - 1)] + geom[4 * (size_t)(n - 1) + 1] * geom[4 * (size_t)(n - 1) + 2] - 1, &at, &tiles) !=
                PP_GEOM_OFFSET_PAST_END || at != n - 1)
            return fail("a short pool not refused", trial, n, at);
        ++cases;
    }
    printf("OK %ld\n", cases);
    return 0;
}
