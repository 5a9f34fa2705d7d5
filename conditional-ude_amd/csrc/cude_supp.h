// Suppression cUDE: what the fixed-step kernels of cude_supp.hip and the dense-output kernel of cude_supp_dense.hip share.
#pragma once
#include "cude_device.h"

namespace cude {

// HA / OA: activation functions other than tanh / softplus (cude_device.h CUDE_GENERAL_ACTS) select the general network
template <int W, int D, int HA, int OA>
struct SuppNetSel { using type = SuppNetG<W, D, HA, OA>; };
template <int W, int D>
struct SuppNetSel<W, D, kActHiddenTanh, kActOutSoftplus> { using type = SuppNet<W, D>; };

// the shape of the reference's experiment with the other activation functions (stage-input mode only)
#define CUDE_SUPP_GENERAL_SHAPES(X) X(3, 5) X(3, 3)

#define CUDE_SUPP_SHAPES(X) X(3, 5) X(3, 2) X(4, 2) X(6, 2) X(5, 2) X(3, 3) X(8, 2) X(3, 4) X(4, 3) X(4, 4) X(5, 3) X(6, 3) X(3, 1) X(4, 1) X(6, 1) X(8, 1)

}  // namespace cude
