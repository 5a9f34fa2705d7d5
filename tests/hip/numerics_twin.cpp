// Host twin of the probe's primitives (tests/hip/numerics_probe.hip): the CUDE_HD functions of csrc/cude_math.h compiled
// by the host compiler, with the same entry points.  The reciprocal seed is the header's host model of v_rcp_f64.
#include "cude_math.h"

using namespace cude;

extern "C" {

// op: as probe_elementwise (0 m_tanh, 1 m_tanh_tab, 2 m_exp2x_t<false>, 3 m_exp2x_t<true>, 4 m_softplus_t<false>,
// 5 m_softplus_t<true>, 6 m_rcp)
int twin_elementwise(int op, const double* x, double* y, double* sig, int n) {
    for (int i = 0; i < n; i++) {
        double s = 0.0, r;
        switch (op) {
            case 0: r = m_tanh(x[i]); break;
            case 1: r = m_tanh_tab(x[i], kTanhTableHost); break;
            case 2: r = m_exp2x_t<false>(x[i]); break;
            case 3: r = m_exp2x_t<true>(x[i]); break;
            case 4: r = m_softplus_t<false>(x[i], &s); break;
            case 5: r = m_softplus_t<true>(x[i], &s); break;
            case 6: r = m_rcp(x[i]); break;
            default: return 1;
        }
        y[i] = r;
        sig[i] = s;
    }
    return 0;
}

int twin_tanh_table(double* out, int n) {
    if (n != kTanhEntries) return 1;
    for (int k = 0; k < kTanhEntries; k++) out[k] = kTanhTableHost[k];
    return 0;
}

}  // extern "C"

template <int W>
void layer_w(int kind, const double* z, double* h, int n) {
    for (int i = 0; i < n; i++) {
        double zz[W], hh[W];
        for (int j = 0; j < W; j++) zz[j] = z[i * W + j];
        if (kind == 0) m_tanh_vec<W>(zz, hh);
        else if (kind == 1) m_tanh_vec_tab<W>(zz, hh, kTanhTableHost);
        else m_tanh_from_exp<W>(zz, hh);
        for (int j = 0; j < W; j++) h[i * W + j] = hh[j];
    }
}

extern "C" {

// the host-compilable layer forms: kind 0 m_tanh_vec, 1 m_tanh_vec_tab, 4 m_tanh_from_exp (probe_layer's kinds)
int twin_layer(int kind, int w, const double* z, double* h, int n) {
    if (kind != 0 && kind != 1 && kind != 4) return 1;
    switch (w) {
        case 1: layer_w<1>(kind, z, h, n); return 0;
        case 2: layer_w<2>(kind, z, h, n); return 0;
        case 3: layer_w<3>(kind, z, h, n); return 0;
        case 4: layer_w<4>(kind, z, h, n); return 0;
        case 5: layer_w<5>(kind, z, h, n); return 0;
        case 6: layer_w<6>(kind, z, h, n); return 0;
        case 7: layer_w<7>(kind, z, h, n); return 0;
        case 8: layer_w<8>(kind, z, h, n); return 0;
    }
    return 1;
}

}  // extern "C"
