// CPU-only driver for the shape dispatch of conditional-ude_amd/csrc/cude_shapes.h, built from that header alone.  Every
// visitor is walked over nin 0..5 x width 0..9 x depth 0..6 (the two-level ones also over hact 0..3 x oact 0..2) and held
// to three things: the callable runs exactly once, with exactly the matching tag, when the shape is in the list; it does
// not run and the not-found value comes back otherwise; and the result is that of the spelling the visitors replaced,
// which is expanded here by hand from the same list macros (#define X ... #undef X).  Built by
// tests/test_shape_dispatch_host.py (plain, and with -fsanitize=address,undefined).  Prints one line per visitor: name, ok
// flag, number of comparisons, number of those in which the shape was in the list.
#include <cstdio>

#include "cude_shapes.h"

namespace {
struct Net {
    int nin, width, depth, hact, oact;
};
constexpr int kNone = -7;          // the not-found value handed to every visitor: no code below is negative

// a shape / an activation pair as one number, from template arguments: the probe below can only form it if the tag's
// members are compile-time constants inside a generic callable that received the tag by value
template <int NIN, int W, int D>
struct ShapeCode {
    static constexpr int value = (NIN * 100 + W) * 100 + D;
};
template <int HA, int OA>
struct ActCode {
    static constexpr int value = HA * 10 + OA;
};
constexpr int shape_code(int nin, int w, int d) { return (nin * 100 + w) * 100 + d; }
constexpr int pair_code(int shape, int ha, int oa) { return shape * 100 + ha * 10 + oa; }

struct Probe {
    int calls = 0;
    template <class S>
    int operator()(S sh) {
        calls++;
        return ShapeCode<sh.nin, sh.width, sh.depth>::value;
    }
    template <class S, class A>
    int operator()(S sh, A act) {
        calls++;
        return pair_code(ShapeCode<sh.nin, sh.width, sh.depth>::value, 0, 0) + ActCode<act.hact, act.oact>::value;
    }
};
struct ActProbe {
    int calls = 0;
    template <class A>
    int operator()(A act) {
        calls++;
        return ActCode<act.hact, act.oact>::value;
    }
};

// ---- the dispatch as it was spelled at the call sites
#define X(NIN, W, D) if (net.nin == NIN && net.width == W && net.depth == D) return shape_code(NIN, W, D);
int old_cpep_shapes(const Net& net) { CUDE_CPEP_SHAPES(X) return kNone; }
int old_cpep_shapes_0(const Net& net) { CUDE_CPEP_SHAPES_0(X) return kNone; }
int old_cpep_shapes_1(const Net& net) { CUDE_CPEP_SHAPES_1(X) return kNone; }
int old_cpep_shapes_2(const Net& net) { CUDE_CPEP_SHAPES_2(X) return kNone; }
int old_cpep_general_shapes(const Net& net) { CUDE_CPEP_GENERAL_SHAPES(X) return kNone; }
#undef X
#define X(W, D) if (net.width == W && net.depth == D) return shape_code(4, W, D);
int old_supp_shapes(const Net& net) { CUDE_SUPP_SHAPES(X) return kNone; }
int old_supp_general_shapes(const Net& net) { CUDE_SUPP_GENERAL_SHAPES(X) return kNone; }
int old_supp_ad_unrolled(const Net& net) { CUDE_SUPP_AD_UNROLLED(X) return kNone; }
int old_supp_ad_shapes(const Net& net) { CUDE_SUPP_AD_SHAPES(X) return kNone; }
#undef X
#define Y(HA, OA) if (hact == HA && oact == OA) return HA * 10 + OA;
int old_general_acts(int hact, int oact) { CUDE_GENERAL_ACTS(Y) return kNone; }
#undef Y
#define Y(HA, OA) if (hact == HA && oact == OA) return true;
bool old_general_acts_compiled(int hact, int oact) { CUDE_GENERAL_ACTS(Y) return false; }
#undef Y
// (the helper templates that held the inner macro: the shape's launch_*_general<NIN, W, D>(net, ...))
#define Y(HA, OA) if (net.hact == HA && net.oact == OA) return pair_code(shape, HA, OA);
int old_general(const Net& net, int shape) { CUDE_GENERAL_ACTS(Y) return kNone; }
#undef Y
#define X(NIN, W, D) if (net.nin == NIN && net.width == W && net.depth == D) return old_general(net, shape_code(NIN, W, D));
int old_cpep_general(const Net& net) { CUDE_CPEP_GENERAL_SHAPES(X) return kNone; }
#undef X
#define X(W, D) if (net.width == W && net.depth == D) return old_general(net, shape_code(4, W, D));
int old_supp_general(const Net& net) { CUDE_SUPP_GENERAL_SHAPES(X) return kNone; }
#undef X

// visit(net, kNone, probe) against old(net) over the grid; model_nin: the tag's nin where the list does not match on it
// (the suppression lists), -1 where the tag's is the net's; pairs: the activation codes are part of the grid and of the tag
template <class Visit, class Old>
bool check(const char* name, Visit visit, Old old, int model_nin, bool pairs) {
    long n_cmp = 0, n_hit = 0;
    bool ok = true;
    for (int nin = 0; nin <= 5; nin++)
        for (int width = 0; width <= 9; width++)
            for (int depth = 0; depth <= 6; depth++)
                for (int hact = 0; hact <= (pairs ? 3 : 0); hact++)
                    for (int oact = 0; oact <= (pairs ? 2 : 0); oact++) {
                        const Net net{nin, width, depth, hact, oact};
                        const int want = old(net);
                        Probe probe;
                        const int got = visit(net, probe);
                        n_cmp++;
                        ok &= got == want && probe.calls == (want == kNone ? 0 : 1);
                        if (want != kNone) {
                            n_hit++;
                            const int shape = shape_code(model_nin < 0 ? nin : model_nin, width, depth);
                            ok &= got == (pairs ? pair_code(shape, hact, oact) : shape);
                        }
                    }
    printf("%s %d %ld %ld\n", name, ok ? 1 : 0, n_cmp, n_hit);
    return ok;
}
#define CHECK(name, model_nin, pairs) \
    check(#name, [](const Net& net, Probe& p) { return cude::visit_##name(net, kNone, p); }, old_##name, model_nin, pairs)
}  // namespace

int main() {
    bool ok = true;
    ok &= CHECK(cpep_shapes, -1, false);
    ok &= CHECK(cpep_shapes_0, -1, false);
    ok &= CHECK(cpep_shapes_1, -1, false);
    ok &= CHECK(cpep_shapes_2, -1, false);
    ok &= CHECK(cpep_general_shapes, -1, false);
    ok &= CHECK(supp_shapes, 4, false);
    ok &= CHECK(supp_general_shapes, 4, false);
    ok &= CHECK(supp_ad_unrolled, 4, false);
    ok &= CHECK(supp_ad_shapes, 4, false);
    ok &= CHECK(cpep_general, -1, true);
    ok &= CHECK(supp_general, 4, true);

    long n_cmp = 0, n_hit = 0;
    bool ok_acts = true, ok_compiled = true;
    for (int hact = 0; hact <= 3; hact++)
        for (int oact = 0; oact <= 2; oact++) {
            const int want = old_general_acts(hact, oact);
            ActProbe probe;
            const int got = cude::visit_general_acts(hact, oact, kNone, probe);
            n_cmp++;
            n_hit += want != kNone;
            ok_acts &= got == want && probe.calls == (want == kNone ? 0 : 1) && (want == kNone || got == hact * 10 + oact);
            ok_compiled &= cude::general_acts_compiled(hact, oact) == old_general_acts_compiled(hact, oact);
        }
    printf("general_acts %d %ld %ld\n", ok_acts ? 1 : 0, n_cmp, n_hit);
    printf("general_acts_compiled %d %ld %ld\n", ok_compiled ? 1 : 0, n_cmp, n_hit);
    return ok && ok_acts && ok_compiled ? 0 : 1;
}
