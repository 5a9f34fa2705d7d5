// Dense output of the fixed-step suppression solve (cude_simulate; SuppArgs::T_data > 0): the states of every subject at
// arbitrary output times, the Tsit5 interpolant of the solve cude_forward runs.
//
// Replaces (reference repo paths):
//   simul(p, prob, individual_data, timepoints) at save times other than the data's   suppression/src/suppression_model.jl:107-115
//   as the figure script calls it on range(0, 30, length = 100)                       suppression/figures.jl:66-74
//
// supp_dense_kernel is the forward sweep of supp_kernel (cude_supp.hip) in the same arithmetic -- the same stage sums,
// the same network body, state 1 from the same closed-form tables (SuppArgs::rho, obs_rho) -- so that at the data times
// it gives cude_forward's trajectory bit for bit; it forms no residual and no reduction.  It is a kernel of its own, in a
// translation unit of its own, so that the code generated for the loss and gradient kernels stays what it was.
//
// Store pattern: one lane per subject.  Written straight into the caller's column-major [3 x T x N], a wave's 64 stores
// of one state and output time land 24 T bytes apart (64 cache lines per instruction, each line filled up by the lane's
// next outputs in L2); the alternative is the lane-contiguous [T][3][N] (traj_sn = 1: one 512-byte row per wave and
// store) reordered by supp_traj_transpose_kernel afterwards.  Either is a matter of the three strides in SuppArgs
// (option "dense_layout"); the direct one measured faster (cude_simulate) and is the default.
#include "cude_device.h"
#include "cude_kernels.h"
#include "cude_supp.h"

namespace cude {

template <int W, int D, int HA, int OA>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1))) void supp_dense_kernel(SuppArgs a) {
    using Net = typename SuppNetSel<W, D, HA, OA>::type;
    extern __shared__ double smem[];
    double* s_K = smem;                  // [7][2] stage derivatives of states 2 and 3 (state 1 is a table lookup)
    const int lane = threadIdx.x;
    const int64_t gid = ((int64_t)blockIdx.x + a.blk_first) * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int64_t N = a.N;
    const int64_t set = blockIdx.y;      // several parameter sets (cude_predictive_bands): one per grid row
    cptr_t p = as_const(a.nn + set * a.set_stride_nn);
    cptr_t obs_w = as_const(a.obs_w);
    cptr_t rho = as_const(a.rho);
    cptr_t obs_rho = as_const(a.obs_rho);
    ciptr_t obs_step = as_const(a.obs_step);
    const int S = a.S, T = a.T, Td = a.T_data;
    const double h = a.h;
#define KROW(j, s) s_K[((j) * 2 + (s)) * kBlock + lane]

    double cst[1] = {exp(a.cond[set * a.set_stride_cond + i])};
    double c[W];
    Net::first_layer_offset(p, cst, c);
#pragma unroll
    for (int j = 0; j < 7; j++)
#pragma unroll
        for (int s = 0; s < 2; s++) KROW(j, s) = 0.0;

    const double u10 = a.data[((int64_t)0 * Td + 0) * N + i];    // u1(t_0): every later u1 is this times a table entry
    double y[2];
#pragma unroll
    for (int s = 0; s < 2; s++) y[s] = a.data[((int64_t)(s + 1) * Td + 0) * N + i];

    // a subject with a non-finite input (theta, u0, a network parameter) gets NaN throughout (the network's tanh table
    // would turn a NaN into finite numbers)
    const bool bad = !(fma(cst[0] + u10 + y[0] + y[1], 0.0, Net::param_check(p)) == 0.0);

    // evaluation e = 0 is k_1 of step 0; e = 6n+st (st = 1..6) is stage st+1 of step n (st = 6: k_7 = f(y_{n+1}))
    int oi = 0, n = 0, st = 0;
    if constexpr (Net::USES_TANH) tanh_tab_init(lane, !Net::LDS_BIAS);
    Net::bias_init(a.nn + set * a.set_stride_nn, lane);
#pragma unroll 1
    for (int e = 0; e <= 6 * S; e++) {
        double u[3];
        u[0] = u10 * rho[e];
        if (st == 0) {
#pragma unroll
            for (int s = 0; s < 2; s++) u[1 + s] = y[s];
        } else {
            double kk[6][2], aj[6];
#pragma unroll
            for (int j = 0; j < 6; j++) {
                aj[j] = TS_A[st][j];
#pragma unroll
                for (int s = 0; s < 2; s++) kk[j][s] = KROW(j, s);
            }
            double t[2] = {0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 6; j++)
#pragma unroll
                for (int s = 0; s < 2; s++) t[s] = fma(aj[j], kk[j][s], t[s]);
#pragma unroll
            for (int s = 0; s < 2; s++) u[1 + s] = fma(h, t[s], y[s]);
        }
        double du[2];
        {
            const double uh = Net::eval(p, c, u);
            du[0] = fma(0.4, u[0], -uh);
            du[1] = fma(-0.3, u[2], uh);
        }
#pragma unroll
        for (int s = 0; s < 2; s++) KROW(st, s) = du[s];
        if (e == 0) { st = 1; continue; }
        if (st < 6) { st++; continue; }
        // ---- end of step n: u = y_{n+1}, KROW(6) = k_7; the outputs inside (t_n, t_{n+1}]
        while (oi < T && obs_step[oi] == n) {
            double o[2] = {0.0, 0.0};
#pragma unroll 1
            for (int j = 0; j < 7; j++) {
                const double w = obs_w[oi * 7 + j];
#pragma unroll
                for (int s = 0; s < 2; s++) o[s] = fma(w, KROW(j, s), o[s]);
            }
            if (active) {
                double* tr = a.traj + set * a.traj_set_stride + oi * a.traj_st + i * a.traj_sn;
                tr[0] = bad ? __builtin_nan("") : u10 * obs_rho[oi];
#pragma unroll
                for (int s = 0; s < 2; s++) tr[(s + 1) * a.traj_ss] = bad ? __builtin_nan("") : fma(h, o[s], y[s]);
            }
            oi++;
        }
#pragma unroll
        for (int s = 0; s < 2; s++) { y[s] = u[1 + s]; KROW(0, s) = du[s]; }
        st = 1;
        n++;
    }
#undef KROW
}

template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
static hipError_t launch_dense(const SuppArgs& a, hipStream_t s) {
    const int64_t nblocks = launch_blocks(a);
    const unsigned n_sets = a.n_sets > 0 ? (unsigned)a.n_sets : 1u;
    if (a.rho == nullptr || a.obs_rho == nullptr || a.traj == nullptr || a.S < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL((supp_dense_kernel<W, D, HA, OA>), dim3((unsigned)nblocks, n_sets), dim3(kBlock),
                       sizeof(double) * (size_t)(7 * 2) * kBlock, s, a);
    return hipGetLastError();
}

hipError_t launch_supp_dense(const NetShape& net, const SuppArgs& a, hipStream_t s) {
    if (net.nin != 4 || net.generic() || a.T_data < 1) return hipErrorInvalidValue;
    if (net.general())
        return visit_supp_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            return launch_dense<sh.width, sh.depth, act.hact, act.oact>(a, s);
        });
    return visit_supp_shapes(net, hipErrorInvalidValue, [&](auto sh) { return launch_dense<sh.width, sh.depth>(a, s); });
}

// the lane-contiguous dense output [T][3][N] into the caller's [N][T][3]: 32 x 32 tiles of the [3T][N] matrix through LDS
__global__ __launch_bounds__(256) void supp_traj_transpose_kernel(int64_t N, int64_t R, const double* __restrict__ src,
                                                                  double* __restrict__ dst) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t c0 = (int64_t)blockIdx.x * 32;
    for (int64_t r0 = (int64_t)blockIdx.y * 32; r0 < R; r0 += (int64_t)gridDim.y * 32) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t r = r0 + ty + 8 * k, c = c0 + tx;
            if (r < R && c < N) tile[ty + 8 * k][tx] = src[r * N + c];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t c = c0 + ty + 8 * k, r = r0 + tx;
            if (r < R && c < N) dst[c * R + r] = tile[tx][ty + 8 * k];
        }
        __syncthreads();
    }
}

hipError_t launch_supp_traj_transpose(int64_t N, int T, const double* src, double* dst, hipStream_t s) {
    const int64_t R = 3 * (int64_t)T;
    const int64_t gy = (R + 31) / 32 < 65535 ? (R + 31) / 32 : 65535;
    hipLaunchKernelGGL(supp_traj_transpose_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)gy), dim3(256), 0, s, N, R, src,
                       dst);
    return hipGetLastError();
}

}  // namespace cude
