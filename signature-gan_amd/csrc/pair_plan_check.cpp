// pair_plan_check.cpp -- a stand-alone host program (no device, not part of the library) that holds pair_plan() of
// pair_plan.h to the two planners it replaced, kept here word for word as ssim.hip and dtw.hip had them, and to what the
// kernels need of a plan: 1 <= S <= 32, whole units per split, no empty split, every column owned.  tests/test_ssim_cpu.py
// builds it with the host compiler under AddressSanitizer and UBSan and runs it.  Prints "OK <cases>" and returns 0, or
// "FAIL ..." and 1.
#include <stdio.h>

#include <vector>

#include "pair_plan.h"

// siggan_ssim_pairs, outside PAIRED mode
static PairPlan ssim_plan(int nb, int row_tiles, int chunk) {
    const int MAX_SPLITS = 32;
    int S = 1, per = nb;
    const int chunks = (nb + chunk - 1) / chunk;
    int want = (1024 + row_tiles - 1) / row_tiles;
    want = want < 1 ? 1 : (want > MAX_SPLITS ? MAX_SPLITS : want);
    want = want > chunks ? chunks : want;
    per = ((chunks + want - 1) / want) * chunk;
    S = (nb + per - 1) / per;
    return {S, per};
}

// siggan_dtw_pairs, outside PAIRED mode
static PairPlan dtw_plan(int nb, int row_tiles) {
    const int MAX_SPLITS = 32;
    int S = 1, per = nb;
    int want = (1024 + row_tiles - 1) / row_tiles;
    want = want < 1 ? 1 : (want > MAX_SPLITS ? MAX_SPLITS : want);
    want = want > nb ? nb : want;
    per = (nb + want - 1) / want;
    S = (nb + per - 1) / per;
    return {S, per};
}

int main() {
    std::vector<int> tiles;
    for (int t = 1; t <= 40; ++t) tiles.push_back(t);
    for (int t : {1023, 1024, 1025, 16384}) tiles.push_back(t);
    long cases = 0;
    for (int unit = 1; unit <= 8; ++unit)
        for (int row_tiles : tiles)
            for (int nb = 1; nb <= 4096; ++nb, ++cases) {
                const PairPlan p = pair_plan(nb, row_tiles, unit);
                const PairPlan s = ssim_plan(nb, row_tiles, unit);
                const PairPlan d = unit == 1 ? dtw_plan(nb, row_tiles) : p;
                const bool sound = p.S >= 1 && p.S <= PAIR_MAX_SPLITS && p.per % unit == 0 && (long)(p.S - 1) * p.per < nb &&
                                   nb <= (long)p.S * p.per;
                if (!sound || p.S != s.S || p.per != s.per || p.S != d.S || p.per != d.per) {
                    printf("FAIL nb = %d, row_tiles = %d, unit = %d: (S, per) = (%d, %d), ssim's (%d, %d), dtw's (%d, %d)\n", nb, row_tiles,
                           unit, p.S, p.per, s.S, s.per, d.S, d.per);
                    return 1;
                }
            }
    printf("OK %ld\n", cases);
    return 0;
}
