// The network shapes and activation pairs the tuned kernels are compiled for, and the ONE dispatch from a run-time shape
// to a compile-time one.  Plain C++17, no HIP: tests/cpp/shape_dispatch.cpp builds this file alone with the host compiler.
//
// Each list is stored as an X-macro and read in two ways, both generated from it by CUDE_SHAPE_LIST below:
//   visit_<list>(net, not_found, f)   tests the list's shapes in the order listed; on the first match returns f(tag), tag
//                                     a ShapeTag carrying the shape as compile-time constants; not_found if none matches.
//                                     `net` is anything with nin / width / depth (NetShape); f takes the tag by value, so
//                                     that tag.width etc. are template arguments inside a generic lambda.
//   count_<list>(nin, width, depth)   how often the list names the shape; size_<list>() its length -- for the static_asserts
//                                     at the end of this file, which hold the lists to what the dispatchers assume of them.
// A shape is compiled for all launches of its model or for none.
#pragma once

namespace cude {

template <int NIN, int W, int D>
struct ShapeTag {
    static constexpr int nin = NIN, width = W, depth = D;
};
template <int HA, int OA>
struct ActTag {
    static constexpr int hact = HA, oact = OA;
};

// c-peptide models, X(inputs, width, hidden layers) -- in three groups, because the longest translation units compile
// one group each (cude_adaptive*.hip -DCUDE_AD_PART=k, cude_refine.hip -DCUDE_REFINE_PART=k)
#define CUDE_CPEP_SHAPES_0(X) X(2, 4, 2) X(2, 6, 2) X(3, 4, 2) X(2, 8, 2) X(2, 4, 3) X(2, 3, 2) X(2, 5, 2) X(2, 7, 2)
#define CUDE_CPEP_SHAPES_1(X) X(3, 6, 2) X(2, 4, 1) X(2, 6, 1) X(2, 6, 3) X(2, 8, 1) X(2, 8, 3) X(3, 8, 2) X(2, 3, 1)
#define CUDE_CPEP_SHAPES_2(X) X(2, 5, 1) X(2, 7, 1) X(2, 3, 3) X(2, 5, 3) X(2, 7, 3) X(3, 4, 1) X(3, 6, 1) X(3, 4, 3)
#define CUDE_CPEP_SHAPES(X) CUDE_CPEP_SHAPES_0(X) CUDE_CPEP_SHAPES_1(X) CUDE_CPEP_SHAPES_2(X)
// ... and those that are also compiled with the other activation functions (CUDE_GENERAL_ACTS)
#define CUDE_CPEP_GENERAL_SHAPES(X) X(2, 4, 2) X(2, 6, 2) X(3, 4, 2)
// suppression model (four inputs), X(width, hidden layers); with the other activation functions: the shapes of the
// reference's experiment (stage-input mode only)
#define CUDE_SUPP_SHAPES(X) X(3, 5) X(3, 2) X(4, 2) X(6, 2) X(5, 2) X(3, 3) X(8, 2) X(3, 4) X(4, 3) X(4, 4) X(5, 3) X(6, 3) X(3, 1) X(4, 1) X(6, 1) X(8, 1)
#define CUDE_SUPP_GENERAL_SHAPES(X) X(3, 5) X(3, 3)
// the adaptive suppression solve: the shapes of the reference's experiments run the unrolled kernel
// (cude_adaptive_unrolled_supp.hip), the others the one-body kernel (cude_adaptive.hip); A/B builds with
// -DCUDE_ADAPT_ONE_BODY compile all of them there
#define CUDE_SUPP_AD_UNROLLED(X) X(3, 5) X(3, 3) X(3, 4) X(3, 2)
#ifdef CUDE_ADAPT_ONE_BODY
#define CUDE_SUPP_AD_SHAPES(X) CUDE_SUPP_SHAPES(X)
#else
#define CUDE_SUPP_AD_SHAPES(X) X(4, 2) X(6, 2) X(5, 2) X(8, 2) X(4, 3) X(4, 4) X(5, 3) X(6, 3) X(3, 1) X(4, 1) X(6, 1) X(8, 1)
#endif
// Networks with other activation functions (Mlp::GENERAL): hidden tanh | relu | sigmoid, output softplus | identity,
// (tanh, softplus) being the specialised default.  Y(hidden, output), codes of cude_kernels.h kActHidden* / kActOut*
#define CUDE_GENERAL_ACTS(Y) Y(0, 1) Y(1, 0) Y(1, 1) Y(2, 0) Y(2, 1)

// (a suppression dispatcher has checked nin == 4 -- or, for the occupancy query, has no need to -- before it looks a
// shape up: its lists match on width and depth alone)
#define CUDE_CPEP_VISIT_(NIN, W, D) if (net.nin == NIN && net.width == W && net.depth == D) return f(ShapeTag<NIN, W, D>{});
#define CUDE_CPEP_COUNT_(NIN, W, D) +(nin == NIN && width == W && depth == D)
#define CUDE_SUPP_VISIT_(W, D) if (net.width == W && net.depth == D) return f(ShapeTag<4, W, D>{});
#define CUDE_SUPP_COUNT_(W, D) +(nin == 4 && width == W && depth == D)
#define CUDE_ONE_(...) +1
#define CUDE_SHAPE_LIST(name, LIST, MODEL)                                                           \
    template <class Net, class R, class F>                                                           \
    inline R visit_##name(const Net& net, R not_found, F&& f) {                                      \
        LIST(CUDE_##MODEL##_VISIT_)                                                                  \
        return not_found;                                                                            \
    }                                                                                                \
    constexpr int count_##name(int nin, int width, int depth) { return 0 LIST(CUDE_##MODEL##_COUNT_); } \
    constexpr int size_##name() { return 0 LIST(CUDE_ONE_); }

CUDE_SHAPE_LIST(cpep_shapes, CUDE_CPEP_SHAPES, CPEP)
CUDE_SHAPE_LIST(cpep_shapes_0, CUDE_CPEP_SHAPES_0, CPEP)
CUDE_SHAPE_LIST(cpep_shapes_1, CUDE_CPEP_SHAPES_1, CPEP)
CUDE_SHAPE_LIST(cpep_shapes_2, CUDE_CPEP_SHAPES_2, CPEP)
CUDE_SHAPE_LIST(cpep_general_shapes, CUDE_CPEP_GENERAL_SHAPES, CPEP)
CUDE_SHAPE_LIST(supp_shapes, CUDE_SUPP_SHAPES, SUPP)
CUDE_SHAPE_LIST(supp_general_shapes, CUDE_SUPP_GENERAL_SHAPES, SUPP)
CUDE_SHAPE_LIST(supp_ad_unrolled, CUDE_SUPP_AD_UNROLLED, SUPP)
CUDE_SHAPE_LIST(supp_ad_shapes, CUDE_SUPP_AD_SHAPES, SUPP)

template <class R, class F>
inline R visit_general_acts(int hact, int oact, R not_found, F&& f) {
#define CUDE_ACT_VISIT_(HA, OA) if (hact == HA && oact == OA) return f(ActTag<HA, OA>{});
    CUDE_GENERAL_ACTS(CUDE_ACT_VISIT_)
#undef CUDE_ACT_VISIT_
    return not_found;
}
inline bool general_acts_compiled(int hact, int oact) {
    return visit_general_acts(hact, oact, false, [](auto) { return true; });
}

// general shape x activation pair (net.hact, net.oact): f(shape tag, activation tag)
template <class Net, class R, class F>
inline R visit_cpep_general(const Net& net, R not_found, F&& f) {
    return visit_cpep_general_shapes(net, not_found, [&](auto shape) {
        return visit_general_acts(net.hact, net.oact, not_found, [&](auto act) { return f(shape, act); });
    });
}
template <class Net, class R, class F>
inline R visit_supp_general(const Net& net, R not_found, F&& f) {
    return visit_supp_general_shapes(net, not_found, [&](auto shape) {
        return visit_general_acts(net.hact, net.oact, not_found, [&](auto act) { return f(shape, act); });
    });
}

#undef CUDE_SHAPE_LIST
#undef CUDE_ONE_
#undef CUDE_SUPP_COUNT_
#undef CUDE_SUPP_VISIT_
#undef CUDE_CPEP_COUNT_
#undef CUDE_CPEP_VISIT_

// ---- what the dispatchers assume of the lists
// pred(nin, width, depth) for every shape of a box that holds all lists (is_set checks that it does)
template <class P>
constexpr bool every_shape(P pred) {
    for (int nin = 0; nin <= 8; nin++)
        for (int width = 0; width <= 16; width++)
            for (int depth = 0; depth <= 8; depth++)
                if (!pred(nin, width, depth)) return false;
    return true;
}
// no shape twice, none outside the box
constexpr bool is_set(int (*count)(int, int, int), int size) {
    int total = 0;
    for (int nin = 0; nin <= 8; nin++)
        for (int width = 0; width <= 16; width++)
            for (int depth = 0; depth <= 8; depth++) {
                if (count(nin, width, depth) > 1) return false;
                total += count(nin, width, depth);
            }
    return total == size;
}
static_assert(is_set(count_cpep_shapes, size_cpep_shapes()) && is_set(count_cpep_shapes_0, size_cpep_shapes_0()) &&
              is_set(count_cpep_shapes_1, size_cpep_shapes_1()) && is_set(count_cpep_shapes_2, size_cpep_shapes_2()) &&
              is_set(count_cpep_general_shapes, size_cpep_general_shapes()) && is_set(count_supp_shapes, size_supp_shapes()) &&
              is_set(count_supp_general_shapes, size_supp_general_shapes()) &&
              is_set(count_supp_ad_unrolled, size_supp_ad_unrolled()) && is_set(count_supp_ad_shapes, size_supp_ad_shapes()),
              "a shape list names a shape twice");
// (the translation units of groups 1 and 2 answer hipErrorNotSupported for a shape of another group, and group 0's asks
// them in turn)
static_assert(size_cpep_shapes() == 24 && every_shape([](int n, int w, int d) {
                  const int in_groups = count_cpep_shapes_0(n, w, d) + count_cpep_shapes_1(n, w, d) + count_cpep_shapes_2(n, w, d);
                  return in_groups <= 1 && in_groups == count_cpep_shapes(n, w, d);
              }),
              "the three c-peptide groups partition CUDE_CPEP_SHAPES");
static_assert(every_shape([](int n, int w, int d) {
                  return count_cpep_general_shapes(n, w, d) <= count_cpep_shapes(n, w, d) &&
                         count_supp_general_shapes(n, w, d) <= count_supp_shapes(n, w, d);
              }),
              "a general-activation shape is one of its model's shapes");
#ifndef CUDE_ADAPT_ONE_BODY
static_assert(size_supp_ad_unrolled() + size_supp_ad_shapes() == size_supp_shapes() && size_supp_shapes() == 16 &&
                  every_shape([](int n, int w, int d) {
                      return count_supp_ad_unrolled(n, w, d) + count_supp_ad_shapes(n, w, d) == count_supp_shapes(n, w, d);
                  }),
              "the unrolled and the one-body adaptive kernel share out CUDE_SUPP_SHAPES");
#endif

}  // namespace cude
