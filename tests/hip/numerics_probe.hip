// Test-only probe of the device arithmetic (tests/test_gpu_numerics.py): the activations of csrc/cude_math.h, the layer
// functions and one network evaluation + reverse sweep of csrc/cude_device.h, run on the device exactly as the product
// kernels compile and run them -- same headers, same flags (csrc/flags.mk), 64-lane workgroups, the parameter vector as
// a kernel argument (wave-uniform: the network reads its weights with scalar loads), the LDS tanh table and LDS biases
// filled before the first evaluation where the network type uses them.  Every entry point copies its inputs to the
// device, launches, synchronises, copies back and returns the hipError_t of the first call that failed.
#include <hip/hip_runtime.h>

#include <vector>

#include "cude_device.h"

using namespace cude;

namespace {

constexpr int kLanes = 64;

// device buffers released on every path out of an entry point
struct Dev {
    std::vector<void*> bufs;
    hipError_t err = hipSuccess;
    ~Dev() {
        for (void* b : bufs) (void)hipFree(b);
    }
    double* up(const double* h, size_t n) {
        double* d = alloc(n);
        if (d && err == hipSuccess && h) err = hipMemcpy(d, h, n * sizeof(double), hipMemcpyHostToDevice);
        return d;
    }
    double* alloc(size_t n) {
        if (err != hipSuccess) return nullptr;
        void* d = nullptr;
        err = hipMalloc(&d, (n ? n : 1) * sizeof(double));
        if (err != hipSuccess) return nullptr;
        bufs.push_back(d);
        err = hipMemset(d, 0, (n ? n : 1) * sizeof(double));
        return (double*)d;
    }
    void down(double* h, const double* d, size_t n) {
        if (err == hipSuccess && h) err = hipMemcpy(h, d, n * sizeof(double), hipMemcpyDeviceToHost);
    }
    void launched() {
        if (err != hipSuccess) return;
        err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
};

int blocks(int n) { return (n + kLanes - 1) / kLanes; }

// ------------------------------------------------------------------------------------ elementwise primitives
enum ElemOp { kTanh = 0, kTanhTab = 1, kExp2x = 2, kExp2xCs = 3, kSoftplus = 4, kSoftplusLone = 5, kRcp = 6 };

template <int OP>
__global__ __launch_bounds__(64) void k_elem(const double* __restrict__ x, double* __restrict__ y,
                                             double* __restrict__ s, int n) {
    const int lane = threadIdx.x;
    if constexpr (OP == kTanhTab) tanh_tab_init(lane);
    const int i = blockIdx.x * kLanes + lane;
    if (i >= n) return;
    const double v = x[i];
    double sig = 0.0, r;
    if constexpr (OP == kTanh) r = m_tanh(v);
    else if constexpr (OP == kTanhTab) r = m_tanh_tab(v, s_tanh_tab);
    else if constexpr (OP == kExp2x) r = m_exp2x_t<false>(v);
    else if constexpr (OP == kExp2xCs) r = m_exp2x_t<true>(v);
    else if constexpr (OP == kSoftplus) r = m_softplus_t<false>(v, &sig);
    else if constexpr (OP == kSoftplusLone) r = m_softplus_t<true>(v, &sig);
    else r = m_rcp(v);
    y[i] = r;
    s[i] = sig;
}

__global__ __launch_bounds__(64) void k_tanh_table(double* __restrict__ out) {
    const int lane = threadIdx.x;
    tanh_tab_init(lane);
    for (int k = lane; k < kTanhEntries; k += kLanes) out[k] = s_tanh_tab[k];
}

// ------------------------------------------------------------------------------------ layer functions
enum LayerKind { kLTanhExp = 0, kLTanhTab = 1, kLRelu = 2, kLSigmoid = 3, kLTanhFromExp = 4 };

template <int W, int KIND>
__global__ __launch_bounds__(64) void k_layer(const double* __restrict__ z, double* __restrict__ h,
                                              double* __restrict__ dh, int n) {
    const int lane = threadIdx.x;
    if constexpr (KIND == kLTanhTab) tanh_tab_init(lane);
    const int i = blockIdx.x * kLanes + lane;
    if (i >= n) return;
    double zz[W], hh[W];
#pragma unroll
    for (int j = 0; j < W; j++) zz[j] = z[i * W + j];
    constexpr int HA = KIND == kLRelu ? kActHiddenRelu : KIND == kLSigmoid ? kActHiddenSigmoid : kActHiddenTanh;
    if constexpr (KIND == kLTanhFromExp) m_tanh_from_exp<W>(zz, hh);
    else act_hidden_vec<W, HA, KIND == kLTanhTab>(zz, hh);
#pragma unroll
    for (int j = 0; j < W; j++) {
        h[i * W + j] = hh[j];
        dh[i * W + j] = act_hidden_deriv<HA>(hh[j]);
    }
}

template <int W, int KIND>
hipError_t run_layer(const double* z, double* h, double* dh, int n) {
    Dev d;
    double* zd = d.up(z, (size_t)n * W);
    double* hd = d.alloc((size_t)n * W);
    double* dd = d.alloc((size_t)n * W);
    if (d.err != hipSuccess) return d.err;
    hipLaunchKernelGGL((k_layer<W, KIND>), dim3(blocks(n)), dim3(kLanes), 0, 0, zd, hd, dd, n);
    d.launched();
    d.down(h, hd, (size_t)n * W);
    d.down(dh, dd, (size_t)n * W);
    return d.err;
}

template <int W>
hipError_t layer_w(int kind, const double* z, double* h, double* dh, int n) {
    switch (kind) {
        case kLTanhExp: return run_layer<W, kLTanhExp>(z, h, dh, n);
        case kLTanhTab: return run_layer<W, kLTanhTab>(z, h, dh, n);
        case kLRelu: return run_layer<W, kLRelu>(z, h, dh, n);
        case kLSigmoid: return run_layer<W, kLSigmoid>(z, h, dh, n);
        case kLTanhFromExp: return run_layer<W, kLTanhFromExp>(z, h, dh, n);
    }
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------ one network evaluation
// Per lane: first_layer_offset, eval, eval_grad with weight 1 from zeroed accumulators, expand.  x[n][NV] are the varying
// inputs, cst[n][NC] the per-subject constants as the network sees them (exp(conditional) [, age]).  use_tab (networks
// with the layer-1 exponent table): the layer-1 exponentials come from anchors exp(2 z_j) formed by tab_anchor.
template <class Net, int NIN>
__global__ __launch_bounds__(64) void k_net(const double* __restrict__ p, const double* __restrict__ x,
                                            const double* __restrict__ cst, int n, int use_tab, double* __restrict__ y_eval,
                                            double* __restrict__ y_grad, double* __restrict__ g,
                                            double* __restrict__ dcond, double* __restrict__ dx) {
    constexpr int NV = NIN - Net::NC, NC = Net::NC, W = Net::WIDTH;
    const int lane = threadIdx.x;
    if constexpr (Net::USES_TANH) tanh_tab_init(lane);
    Net::bias_init(p, lane);
    const int i = blockIdx.x * kLanes + lane;
    if (i >= n) return;
    const cptr_t cp = as_const(p);
    double xv[NV], cs[NC > 0 ? NC : 1];
#pragma unroll
    for (int k = 0; k < NV; k++) xv[k] = x[i * NV + k];
#pragma unroll
    for (int k = 0; k < NC; k++) cs[k] = cst[i * NC + k];
    double c[W];
    Net::first_layer_offset(cp, cs, c);
    typename Net::Exps E;
    bool tab = false;
    if constexpr (Net::HAS_TAB) {
        if (use_tab) {
            Net::tab_anchor(cp, c, xv[0], E);
            tab = true;
        }
    }
    y_eval[i] = Net::eval(cp, c, xv, tab, &E);
    double acc[Net::NACC];
#pragma unroll
    for (int q = 0; q < Net::NACC; q++) acc[q] = 0.0;
    double dxv[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) dxv[k] = 0.0;
    y_grad[i] = Net::template eval_grad<true>(cp, c, xv, 1.0, acc, dxv, tab, &E);
    double gg[Net::P], dc;
    Net::expand(cp, acc, cs, gg, &dc);
#pragma unroll
    for (int q = 0; q < Net::P; q++) g[(size_t)i * Net::P + q] = gg[q];
    dcond[i] = dc;
#pragma unroll
    for (int k = 0; k < NV; k++) dx[i * NV + k] = dxv[k];
}

// param_check of parameter set b (one workgroup per set: the set's base address is wave-uniform)
template <class Net>
__global__ __launch_bounds__(64) void k_param_check(const double* __restrict__ p, double* __restrict__ out) {
    const double* pb = p + (size_t)blockIdx.x * Net::P;
    const double r = Net::param_check(as_const(pb));
    out[blockIdx.x * kLanes + threadIdx.x] = r;
}

template <class Net, int NIN>
hipError_t run_net(const double* p, const double* x, const double* cst, int n, int use_tab, double* y_eval,
                   double* y_grad, double* g, double* dcond, double* dx) {
    constexpr int NV = NIN - Net::NC, NC = Net::NC;
    Dev d;
    double* pd = d.up(p, Net::P);
    double* xd = d.up(x, (size_t)n * NV);
    double* cd = d.up(cst, (size_t)n * NC);
    double* ye = d.alloc(n);
    double* yg = d.alloc(n);
    double* gd = d.alloc((size_t)n * Net::P);
    double* dcd = d.alloc(n);
    double* dxd = d.alloc((size_t)n * NV);
    if (d.err != hipSuccess) return d.err;
    hipLaunchKernelGGL((k_net<Net, NIN>), dim3(blocks(n)), dim3(kLanes), 0, 0, pd, xd, cd, n, use_tab, ye, yg, gd, dcd,
                       dxd);
    d.launched();
    d.down(y_eval, ye, n);
    d.down(y_grad, yg, n);
    d.down(g, gd, (size_t)n * Net::P);
    d.down(dcond, dcd, n);
    d.down(dx, dxd, (size_t)n * NV);
    return d.err;
}

template <class Net>
hipError_t run_param_check(const double* p, int n_sets, double* out) {
    Dev d;
    double* pd = d.up(p, (size_t)n_sets * Net::P);
    double* od = d.alloc((size_t)n_sets * kLanes);
    if (d.err != hipSuccess) return d.err;
    hipLaunchKernelGGL((k_param_check<Net>), dim3(n_sets), dim3(kLanes), 0, 0, pd, od);
    d.launched();
    std::vector<double> all((size_t)n_sets * kLanes);
    d.down(all.data(), od, all.size());
    if (d.err != hipSuccess) return d.err;
    // every lane of a workgroup reads the same parameters: they must agree (NaN with NaN)
    for (int b = 0; b < n_sets; b++) {
        const double r0 = all[(size_t)b * kLanes];
        for (int l = 1; l < kLanes; l++) {
            const double r = all[(size_t)b * kLanes + l];
            if (!(r == r0 || (r != r && r0 != r0))) return hipErrorUnknown;
        }
        out[b] = r0;
    }
    return hipSuccess;
}

// the networks the product kernels are compiled for (csrc/cude_shapes.h CUDE_CPEP_SHAPES, CUDE_SUPP_SHAPES;
// CUDE_CPEP_GENERAL_SHAPES / CUDE_SUPP_GENERAL_SHAPES x CUDE_GENERAL_ACTS, one shape per pair)
enum Family { kCpep = 0, kSupp = 1, kCpepG = 2, kSuppG = 3 };

// calls F<Net, NIN>::run(args...) for the network (family, nin, w, d, ha, oa); hipErrorInvalidValue if it is not compiled
template <template <class, int> class F, class... Args>
hipError_t dispatch(int family, int nin, int w, int dd, int ha, int oa, Args... args) {
#define C1(NIN, W, D) \
    if (family == kCpep && nin == NIN && w == W && dd == D && ha == 0 && oa == 0) return F<CpepNet<NIN, W, D>, NIN>::run(args...);
    CUDE_CPEP_SHAPES(C1)
#undef C1
#define S1(W, D) \
    if (family == kSupp && nin == 4 && w == W && dd == D && ha == 0 && oa == 0) return F<SuppNet<W, D>, 4>::run(args...);
    CUDE_SUPP_SHAPES(S1)
#undef S1
#define G1(HA, OA)                                                                            \
    if (family == kCpepG && nin == 2 && w == 4 && dd == 2 && ha == HA && oa == OA)            \
        return F<CpepNetG<2, 4, 2, HA, OA>, 2>::run(args...);                                 \
    if (family == kSuppG && nin == 4 && w == 3 && dd == 5 && ha == HA && oa == OA)            \
        return F<SuppNetG<3, 5, HA, OA>, 4>::run(args...);
    CUDE_GENERAL_ACTS(G1)
#undef G1
    return hipErrorInvalidValue;
}

template <class Net, int NIN>
struct NetRun {
    static hipError_t run(const double* p, const double* x, const double* cst, int n, int use_tab, double* y_eval,
                          double* y_grad, double* g, double* dcond, double* dx) {
        return run_net<Net, NIN>(p, x, cst, n, use_tab, y_eval, y_grad, g, dcond, dx);
    }
};
template <class Net, int NIN>
struct CheckRun {
    static hipError_t run(const double* p, int n_sets, double* out) { return run_param_check<Net>(p, n_sets, out); }
};
template <class Net, int NIN>
struct InfoRun {
    static hipError_t run(int* info) {
        info[0] = Net::P;
        info[1] = Net::HAS_TAB ? 1 : 0;
        info[2] = Net::TT ? 1 : 0;
        info[3] = Net::LDS_BIAS ? 1 : 0;
        return hipSuccess;
    }
};

}  // namespace

extern "C" {

// y[i] = op(x[i]); sig[i] = the logistic derivative (softplus ops), 0 otherwise.  op: ElemOp.
int probe_elementwise(int op, const double* x, double* y, double* sig, int n) {
    Dev d;
    double* xd = d.up(x, n);
    double* yd = d.alloc(n);
    double* sd = d.alloc(n);
    if (d.err != hipSuccess) return d.err;
    const dim3 g(blocks(n)), b(kLanes);
    switch (op) {
        case kTanh: hipLaunchKernelGGL(k_elem<kTanh>, g, b, 0, 0, xd, yd, sd, n); break;
        case kTanhTab: hipLaunchKernelGGL(k_elem<kTanhTab>, g, b, 0, 0, xd, yd, sd, n); break;
        case kExp2x: hipLaunchKernelGGL(k_elem<kExp2x>, g, b, 0, 0, xd, yd, sd, n); break;
        case kExp2xCs: hipLaunchKernelGGL(k_elem<kExp2xCs>, g, b, 0, 0, xd, yd, sd, n); break;
        case kSoftplus: hipLaunchKernelGGL(k_elem<kSoftplus>, g, b, 0, 0, xd, yd, sd, n); break;
        case kSoftplusLone: hipLaunchKernelGGL(k_elem<kSoftplusLone>, g, b, 0, 0, xd, yd, sd, n); break;
        case kRcp: hipLaunchKernelGGL(k_elem<kRcp>, g, b, 0, 0, xd, yd, sd, n); break;
        default: return hipErrorInvalidValue;
    }
    d.launched();
    d.down(y, yd, n);
    d.down(sig, sd, n);
    return d.err;
}

// the LDS tanh table as tanh_tab_init leaves it: kTanhEntries doubles
int probe_tanh_table(double* out, int n) {
    if (n != kTanhEntries) return hipErrorInvalidValue;
    Dev d;
    double* od = d.alloc(kTanhEntries);
    if (d.err != hipSuccess) return d.err;
    hipLaunchKernelGGL(k_tanh_table, dim3(1), dim3(kLanes), 0, 0, od);
    d.launched();
    d.down(out, od, kTanhEntries);
    return d.err;
}

// one layer of W units per lane: h = activation(z) (kind: LayerKind; kLTanhFromExp takes E = exp(2 z) as input),
// dh = act_hidden_deriv(h).  z, h, dh: [n][W]
int probe_layer(int kind, int w, const double* z, double* h, double* dh, int n) {
    switch (w) {
        case 1: return layer_w<1>(kind, z, h, dh, n);
        case 2: return layer_w<2>(kind, z, h, dh, n);
        case 3: return layer_w<3>(kind, z, h, dh, n);
        case 4: return layer_w<4>(kind, z, h, dh, n);
        case 5: return layer_w<5>(kind, z, h, dh, n);
        case 6: return layer_w<6>(kind, z, h, dh, n);
        case 7: return layer_w<7>(kind, z, h, dh, n);
        case 8: return layer_w<8>(kind, z, h, dh, n);
    }
    return hipErrorInvalidValue;
}

// info[0..3] = P, HAS_TAB, TT (table tanh), LDS_BIAS of a compiled network; nonzero if it is not compiled
int probe_net_info(int family, int nin, int w, int d, int ha, int oa, int* info) {
    return dispatch<InfoRun>(family, nin, w, d, ha, oa, info);
}

// see k_net.  g: [n][P] in SimpleChains order; dx: [n][NV]
int probe_net(int family, int nin, int w, int d, int ha, int oa, const double* p, const double* x, const double* cst,
              int n, int use_tab, double* y_eval, double* y_grad, double* g, double* dcond, double* dx) {
    return dispatch<NetRun>(family, nin, w, d, ha, oa, p, x, cst, n, use_tab, y_eval, y_grad, g, dcond, dx);
}

// out[b] = param_check(p + b * P) for n_sets parameter sets
int probe_param_check(int family, int nin, int w, int d, int ha, int oa, const double* p, int n_sets, double* out) {
    return dispatch<CheckRun>(family, nin, w, d, ha, oa, p, n_sets, out);
}

}  // extern "C"
