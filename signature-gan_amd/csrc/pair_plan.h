// pair_plan.h -- how the ops that score every image of a set a against every image of a set b (image_pairs.h) split b's
// columns over gridDim.y.  No HIP in it: it compiles with -x c++, which is how pair_plan_check.cpp holds it to the two formulas it replaced.
#pragma once

constexpr int PAIR_MAX_SPLITS = 32, PAIR_WORKGROUPS = 1024;    // the workgroups aimed at: enough for every CU a few times over

struct PairPlan { int S, per; };         // split s owns columns [s * per, min(nb, (s + 1) * per))

// nb >= 1 columns, row_tiles >= 1 workgroups along the rows; `unit`: the number of b-images a split's extent is a multiple
// of (the chunk a kernel stages at a time; 1 where it stages none).  No split is empty and every column is owned.
inline PairPlan pair_plan(int nb, int row_tiles, int unit) {
    const int units = (nb + unit - 1) / unit;
    int want = (PAIR_WORKGROUPS + row_tiles - 1) / row_tiles;
    want = want < 1 ? 1 : (want > PAIR_MAX_SPLITS ? PAIR_MAX_SPLITS : want);
    want = want > units ? units : want;
    const int per = ((units + want - 1) / want) * unit;
    return {(nb + per - 1) / per, per};
}
