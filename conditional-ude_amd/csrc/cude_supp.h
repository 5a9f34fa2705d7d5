// Suppression cUDE: what the fixed-step kernels of cude_supp.hip and the dense-output kernel of cude_supp_dense.hip share.
#pragma once
#include "cude_device.h"

namespace cude {

// HA / OA: activation functions other than tanh / softplus (cude_shapes.h CUDE_GENERAL_ACTS) select the general network
template <int W, int D, int HA, int OA>
struct SuppNetSel { using type = SuppNetG<W, D, HA, OA>; };
template <int W, int D>
struct SuppNetSel<W, D, kActHiddenTanh, kActOutSoftplus> { using type = SuppNet<W, D>; };

}  // namespace cude
