// Host arithmetic that needs no context and no HIP runtime, so that a host test can include it (tests/cpp/replicate_passes.cpp):
// the passes over whole workgroups of subjects of cude_predictive_bands, cude_bootstrap_conditional and cude_npde, and their
// check of a list of ranks.
#pragma once
#include <algorithm>
#include <cstdint>

namespace cude {
namespace api {

// Subjects per pass: whole workgroups of `width` subjects, as many as the budget holds at bytes_per_block each, at least
// one; an option that names a count of subjects (rounded up to whole workgroups; tests force several passes with it)
// replaces the budget's answer.  Pass b0 = 0, blocks, 2 blocks ... < nb takes workgroups [b0, b0 + bn) = subjects
// [s0, s0 + sn); sub_max is the largest sn.
struct SubjectPasses {
    int64_t N = 0, nb = 0, width = 0;
    int64_t blocks = 0, sub_max = 0;
    struct Pass { int64_t b0, bn, s0, sn; };
    Pass at(int64_t b0) const {
        const int64_t bn = std::min<int64_t>(blocks, nb - b0);
        const int64_t s0 = b0 * width;
        return {b0, bn, s0, std::min<int64_t>(N, (b0 + bn) * width) - s0};
    }
};
inline SubjectPasses subject_passes(int64_t N, int64_t nb, int64_t width, double budget_bytes, double bytes_per_block,
                                    int option_subjects) {
    SubjectPasses p;
    p.N = N; p.nb = nb; p.width = width;
    p.blocks = std::max<int64_t>(1, std::min<int64_t>(nb, (int64_t)(budget_bytes / bytes_per_block)));
    if (option_subjects > 0) p.blocks = std::min<int64_t>(nb, ((int64_t)option_subjects + width - 1) / width);
    p.sub_max = std::min<int64_t>(N, p.blocks * width);
    return p;
}

// ranks strictly increasing inside [0, n)
inline bool ranks_increasing(int32_t n_ranks, const int32_t* ranks, int32_t n) {
    for (int32_t r = 0; r < n_ranks; r++)
        if (ranks[r] < 0 || ranks[r] >= n || (r > 0 && ranks[r] <= ranks[r - 1])) return false;
    return true;
}

}  // namespace api
}  // namespace cude
