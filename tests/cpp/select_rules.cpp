// CPU-only driver for the context-free launch rules of conditional-ude_amd/csrc/cude_select.hip: sets_per_launch,
// nearest_divisor and shared_simd_rate, compiled from that file itself (CUDE_SELECT_RULES_ONLY leaves out everything that
// needs a context or the HIP runtime).  Each is compared, over a grid of inputs, with the expression it replaced at its
// call sites, written out here as it stood there.  Built by tests/test_select_rules_host.py (plain, and with
// -fsanitize=address,undefined).  Prints one line per rule: name, ok flag, number of comparisons.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#define CUDE_SELECT_RULES_ONLY
#include "cude_select.hip"

using cude::api::chunk_starts;
using cude::api::nearest_divisor;
using cude::api::shared_simd_rate;

namespace {
constexpr int64_t kNoGridCap = std::numeric_limits<int64_t>::max();
constexpr int T = 8, NS = 3, L = 5, S30 = 30;       // population constants of the per-set byte counts below

// (the default of the declaration in cude_ctx.h)
int64_t sets_per_launch(int64_t n, int64_t grid_cap, double budget_bytes, double bytes_per_set, int option_cap = 0) {
    return cude::api::sets_per_launch(n, grid_cap, budget_bytes, bytes_per_set, option_cap);
}

long n_cmp = 0;
bool same(int64_t got, int64_t want) {
    n_cmp++;
    return got == want;
}

// ---- the expressions as they stood at the call sites
int64_t old_capped(int64_t n, double budget_over_per_set_arg, double per, int cap) {      // profile / scores / info
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n, 32768), (int64_t)(budget_over_per_set_arg / per)));
    if (cap > 0) chunk = std::min<int64_t>(chunk, cap);
    return chunk;
}
int64_t old_eval_sets(int64_t n_sets, bool split, double budget, double per_set) {
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_sets, split ? 16384 : 32768), (int64_t)(budget / per_set)));
}
int64_t old_multistart(int64_t n_sets, int64_t nb, int P) {
    int64_t chunk = std::min<int64_t>(n_sets, 32768);
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(256e6 / ((double)nb * (P + 2) * 8.0))));
    return chunk;
}
int64_t old_screen(int64_t n_candidates, int64_t nb, int P, int64_t N) {
    int64_t chunk = std::min<int64_t>(n_candidates, 32768);
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(256e6 / ((double)nb * (P + 2) * 8.0))));
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(512e6 / ((double)(P + N) * 8.0))));
    return chunk;
}
int old_fit_grid(int n_grid, double per_set) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(n_grid, (int64_t)(256e6 / per_set)));
}
int64_t old_simulate(int64_t n_times, int64_t N, int dense_chunk) {
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_times, (int64_t)(1e9 / (8.0 * NS * (double)N))));
    if (dense_chunk > 0) chunk = std::min<int64_t>(chunk, dense_chunk);
    return chunk;
}
int old_nearest(int S, double target) {
    int Lm = 0;
    for (int d = 2; d <= S; d++)
        if (S % d == 0 && (Lm == 0 || std::fabs(d - target) < std::fabs(Lm - target))) Lm = d;
    return Lm;
}
double old_rate(double w) { return w <= 1.0 ? 1.0 : (w <= 2.0 ? 1.33 : (w <= 3.0 ? 1.36 : 1.38)); }
}  // namespace

int main() {
    const int64_t ns[] = {1, 2, 37, 32768, 1000000};
    const int64_t Ns[] = {1, 57, 64, 65, 100000, 1000000};
    const int Ps[] = {13, 67, 1291};
    const double budgets[] = {256e6, 512e6, 16e9};
    const int caps[] = {0, 1, 8, 333};
    bool ok = true;
    for (int64_t n : ns)
        for (int64_t N : Ns)
            for (int P : Ps) {
                const int64_t nb = (N + 63) / 64;
                // cude_multistart_forward, cude_screen_candidates (two budgets in sequence), cude_fit_conditional's grid
                ok &= same(sets_per_launch(n, 32768, 256e6, (double)nb * (P + 2) * 8.0), old_multistart(n, nb, P));
                ok &= same(sets_per_launch(sets_per_launch(n, 32768, 256e6, (double)nb * (P + 2) * 8.0), 32768, 512e6, (double)(P + N) * 8.0),
                           old_screen(n, nb, P, N));
                for (int fsplit = 0; fsplit < 2; fsplit++) {
                    const double per_set = 8.0 * ((double)N * (2 + (fsplit ? (double)L * (3 + T) : 0.0)) + (double)nb * (P + 2));
                    ok &= same(sets_per_launch(n, kNoGridCap, 256e6, per_set), old_fit_grid((int)n, per_set));
                }
                for (int cap : caps) {
                    // profile_chunk_sets, cude_simulate
                    const double per_point = 8.0 * (2.0 * N + (double)nb * (P + 2));
                    ok &= same(sets_per_launch(n, 32768, 512e6, per_point, cap), old_capped(n, 512e6, per_point, cap));
                    ok &= same(sets_per_launch(n, kNoGridCap, 1e9, 8.0 * NS * (double)N, cap), old_simulate(n, N, cap));
                    for (double B : budgets) {
                        // scores_chunk_sets, info_chunk_sets (with and without the staging)
                        const double per_score = 8.0 * ((double)P + 4.0) * (double)N;
                        ok &= same(sets_per_launch(n, 32768, 0.5 * B, per_score, cap), old_capped(n, 0.5 * B, per_score, cap));
                        for (int stage = 0; stage < 2; stage++) {
                            const double per_info = 8.0 * ((stage ? 2.5 : 1.0) * (double)P + 3.0) * (double)N;
                            ok &= same(sets_per_launch(n, 32768, 0.5 * B, per_info, cap), old_capped(n, 0.5 * B, per_info, cap));
                        }
                    }
                }
                for (double B : budgets)
                    for (int split = 0; split < 2; split++) {       // eval_sets_device: a fixed-step launch, plain and time-split
                        const double per_set =
                            8.0 * ((double)nb * (P + 2) +
                                   (split ? (double)L * (3 + T) * N + 5.0 * S30 * N + (double)L * N + (double)L * nb * P : 0.0));
                        ok &= same(sets_per_launch(n, split ? 16384 : 32768, B, per_set), old_eval_sets(n, split != 0, B, per_set));
                    }
            }
    printf("sets_per_launch %d %ld\n", ok ? 1 : 0, n_cmp);

    n_cmp = 0;
    bool ok_div = true, ok_starts = true;
    for (int S : {1, 7, 30, 60})
        for (double target : {S / 3.0, S / 6.0}) {
            ok_div &= same(nearest_divisor(S, target), old_nearest(S, target));
            const int d = std::max(1, nearest_divisor(S, target));
            const std::vector<int32_t> cs = chunk_starts(S, d);
            ok_starts &= (int)cs.size() == d + 1 && cs.front() == 0 && cs.back() == S;
            for (int k = 0; k <= d; k++) ok_starts &= cs[k] == (int32_t)((int64_t)k * S / d);
        }
    printf("nearest_divisor %d %ld\n", ok_div ? 1 : 0, n_cmp);
    printf("chunk_starts %d %d\n", ok_starts ? 1 : 0, 8);

    n_cmp = 0;
    bool ok_rate = true;
    for (double w : {0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 17.0}) {
        n_cmp++;
        ok_rate &= shared_simd_rate(w) == old_rate(w);
    }
    printf("shared_simd_rate %d %ld\n", ok_rate ? 1 : 0, n_cmp);
    return ok && ok_div && ok_starts && ok_rate ? 0 : 1;
}
