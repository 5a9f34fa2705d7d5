// CPU-only driver for the host arithmetic the replicate-simulation entry points share: tile_geometry of
// conditional-ude_amd/csrc/cude_tilesort.h (CUDE_TILE_GEOMETRY_ONLY leaves out the device functions and the HIP runtime) and
// the subject passes and the rank check of csrc/cude_passes.h.  The geometry is compared with the table that
// tests/test_tilesort_host.py states; the passes with the expressions of cude_predictive_bands, cude_bootstrap_conditional
// and cude_npde as they stood at their call sites, written out here, and with what a set of passes must be: [0, N) exactly
// once, in order, every start a multiple of 64.  Built by tests/test_replicate_passes_host.py (plain, and with
// -fsanitize=address,undefined).  Prints one line per rule: name, ok flag, number of comparisons.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#define CUDE_TILE_GEOMETRY_ONLY
#include "cude_passes.h"
#include "cude_tilesort.h"

using cude::api::ranks_increasing;
using cude::api::subject_passes;
using cude::api::SubjectPasses;

namespace {
constexpr int64_t kBlock = 64;
constexpr int T = 8, NS = 3;        // population constants of the per-workgroup byte counts below

long n_cmp = 0;
bool same(int64_t got, int64_t want) {
    n_cmp++;
    return got == want;
}

// ---- the expressions as they stood at the three call sites: blocks per pass, then the largest pass
int64_t old_blocks(int64_t nb, double budget_over_per_block, int option_subjects) {
    int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(nb, (int64_t)budget_over_per_block));
    if (option_subjects > 0) blocks = std::min<int64_t>(nb, ((int64_t)option_subjects + kBlock - 1) / kBlock);
    return blocks;
}

// the passes against the loop of the call sites; covering
bool check_passes(const SubjectPasses& p, int64_t N, int64_t nb, int64_t blocks) {
    bool ok = same(p.blocks, blocks) & same(p.sub_max, std::min<int64_t>(N, blocks * kBlock));
    int64_t next = 0, largest = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += blocks) {
        const int64_t bn = std::min<int64_t>(blocks, nb - b0);
        const int64_t s0 = b0 * kBlock, sn = std::min<int64_t>(N, (b0 + bn) * kBlock) - s0;
        const SubjectPasses::Pass q = p.at(b0);
        ok &= same(q.b0, b0) & same(q.bn, bn) & same(q.s0, s0) & same(q.sn, sn);
        ok &= q.s0 == next && q.s0 % kBlock == 0 && q.sn >= 1 && q.bn >= 1;
        next = q.s0 + q.sn;
        largest = std::max(largest, q.sn);
    }
    return ok && next == N && largest == p.sub_max;
}
}  // namespace

int main() {
    // ---- the tile: (Kp, C) of tests/test_tilesort_host.py's table, C = 1 << lgC, lds = 8 Kp C
    const int table[][3] = {{1, 1, 64},      {2, 2, 64},      {3, 4, 64},      {64, 64, 64},     {65, 128, 64},  {129, 256, 32},
                            {257, 512, 16},  {513, 1024, 8},  {1025, 2048, 4}, {2049, 4096, 2},  {4096, 4096, 2}};
    bool ok_geo = true;
    for (const auto& row : table) {
        const cude::TileGeometry g = cude::tile_geometry(row[0]);
        ok_geo &= same(g.Kp, row[1]) & same(g.C, row[2]) & same(1 << g.lgC, g.C) & same((int64_t)g.lds, 8 * (int64_t)row[1] * row[2]);
        ok_geo &= g.lds <= sizeof(double) * cude::kTileSortDoubles;
    }
    printf("tile_geometry %d %ld\n", ok_geo ? 1 : 0, n_cmp);

    // ---- the passes.  Per-workgroup bytes of the three sites at K sets / replicates / simulations; budgets that give one
    // workgroup per pass, a few, and all of them
    n_cmp = 0;
    bool ok_pass = true;
    const int64_t Ns[] = {1, 57, 64, 65, 700, 100000};
    const int caps[] = {0, 1, 64, 65, 1000};
    const int Ks[] = {2, 1000, 4096};
    long n_sets = 0;
    for (int64_t N : Ns)
        for (int cap : caps)
            for (int K : Ks)
                for (int few = 0; few < 3; few++) {
                    const int64_t nb = (N + kBlock - 1) / kBlock;
                    // cude_predictive_bands: Tc output times of NS states of K sets
                    const int64_t Tc = 5;
                    const double per_time = 8.0 * NS * (double)K * kBlock;
                    // cude_bootstrap_conditional: a double and an int32 per replicate
                    const double per_boot = 12.0 * K * kBlock;
                    // cude_npde: trajectories, simulated observations and flags
                    const int R = T - 1;
                    const double per_npde = ((8.0 * NS * T + 8.0 * R + 1.0) * (double)K) * kBlock;
                    const double pers[] = {per_time * (double)Tc, per_boot, per_npde};
                    for (double per : pers) {
                        // one workgroup (the budget holds less than one), three, all (the sites' own 1e9 at N <= 700)
                        const double budget = few == 0 ? 0.5 * per : (few == 1 ? 3.5 * per : 1e9);
                        const SubjectPasses p = subject_passes(N, nb, kBlock, budget, per, cap);
                        ok_pass &= check_passes(p, N, nb, old_blocks(nb, budget / per, cap));
                        n_sets++;
                    }
                }
    printf("subject_passes %d %ld %ld\n", ok_pass ? 1 : 0, n_cmp, n_sets);

    // ---- ranks: strictly increasing inside [0, n)
    n_cmp = 0;
    const int32_t good[] = {0, 3, 8}, dup[] = {0, 3, 3}, down[] = {3, 0, 8}, neg[] = {-1, 3, 8};
    bool ok_rank = same(ranks_increasing(0, nullptr, 9), 1) & same(ranks_increasing(3, good, 9), 1) &&
                   same(ranks_increasing(3, good, 8), 0) & same(ranks_increasing(3, dup, 9), 0) &&
                   same(ranks_increasing(3, down, 9), 0) & same(ranks_increasing(3, neg, 9), 0);
    printf("ranks_increasing %d %ld\n", ok_rank ? 1 : 0, n_cmp);
    return ok_geo && ok_pass && ok_rank ? 0 : 1;
}
