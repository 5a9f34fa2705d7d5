"""The branch-free fp64 activations of the kernels (csrc/cude_math.h) compiled for the host and compared with
libm.  (On the device the reciprocal seed is v_rcp_f64 instead of a float division; both are refined to
full precision by Newton steps.)"""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "cude_math.h"
#include <cstdio>
#include <cmath>
#include <random>
int main(){
  std::mt19937_64 g(1); std::uniform_real_distribution<double> U(-1,1);
  double et=0, es=0, eg=0, ee=0;
  for(int i=0;i<2000000;i++){
    double s = std::pow(10.0, 3*U(g)-1.5); double x = U(g)*s*20;
    et=fmax(et,fabs(cude::m_tanh(x)-tanh(x)));
    double sg; double sp=cude::m_softplus(x,&sg);
    double ref = x>30? x + log1p(exp(-x)) : log1p(exp(x));
    es=fmax(es,fabs(sp-ref)/fmax(1.0,fabs(ref))); eg=fmax(eg,fabs(sg-1.0/(1.0+exp(-x))));
    double y=U(g)*40; ee=fmax(ee,fabs(cude::m_exp(y)/exp(y)-1));
  }
  double ev=0;
  for(int i=0;i<300000;i++){
    double z[6], t[6]; for(int j=0;j<6;j++){ double s = std::pow(10.0, 3*U(g)-1.5); z[j]=U(g)*s*20; }
    cude::m_tanh_vec<6>(z,t); for(int j=0;j<6;j++) ev=fmax(ev,fabs(t[j]-tanh(z[j])));
  }
  printf("%.6g %.6g %.6g %.6g %.6g\n",et,es,eg,ee,ev);
  double sg;
  printf("%.17g %.17g %.17g %.17g\n", cude::m_tanh(0.0), cude::m_tanh(900.0), cude::m_tanh(-1e9), cude::m_softplus(800.0,&sg));
}
'''


def test_activation_accuracy():
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(SRC)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-O2", "-I", os.path.join(ROOT, "conditional-ude_amd", "csrc"),
                               os.path.join(d, "t.cpp"), "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    et, es, eg, ee, ev = (float(v) for v in out[0].split())
    assert et < 5e-16 and es < 8e-16 and eg < 6e-16 and ee < 6e-16 and ev < 2e-15
    t0, tbig, tneg, spbig = (float(v) for v in out[1].split())
    assert t0 == 0.0 and tbig == 1.0 and tneg == -1.0 and spbig == 800.0


# ---- the host twin of the numerics probe (tests/hip/numerics_twin.cpp): the primitives the kernels use, against 50-digit
# references on the probe's inputs (grid points and midpoints of the tanh table +-2 ulp, clamps, range-reduction switch
# points, the softplus branch, zeros, subnormals, infinities).  The device must meet the same bars
# (tests/test_gpu_numerics.py).
def test_host_twin_against_50_digits():
    import numpy as np
    import numerics_ref as nr
    nr.build("libnumerics_twin.so", timeout=120)
    tw = nr.load_twin()
    for op in range(len(nr.OP_NAMES)):
        x = nr.elementwise_inputs(op)
        y, s = nr.elementwise(tw.twin_elementwise, op, x)
        ev, es = nr.elementwise_errors(op, x, y, s)
        bar_v, bar_s = nr.ELEM_BARS[op]
        assert ev.max() <= bar_v, (nr.OP_NAMES[op], x[np.argmax(ev)], ev.max())
        if bar_s is not None:
            assert es.max() <= bar_s, (nr.OP_NAMES[op], x[np.argmax(es)], es.max())
        if op in (nr.TANH, nr.TANH_TAB):
            z = np.array([0.0, -0.0])
            assert np.array_equal(np.signbit(nr.elementwise(tw.twin_elementwise, op, z)[0]), [False, True])
    table = np.empty(161)
    assert tw.twin_tanh_table(nr.ptr(table), 161) == 0
    assert np.array_equal(table.view(np.int64), nr.tanh_table_reference().view(np.int64))
    for kind in (nr.L_TANH_EXP, nr.L_TANH_TAB, nr.L_TANH_FROM_EXP):
        for W in range(1, 9):
            z = nr.layer_inputs(kind, W)
            h = np.empty_like(z)
            assert tw.twin_layer(kind, W, nr.ptr(z), nr.ptr(h), z.shape[0]) == 0
            href, dref = nr.layer_reference(kind, z)
            assert np.abs(h - href).max() <= nr.LAYER_BARS[kind], (nr.LAYER_NAMES[kind], W)
            assert np.abs(nr.tanh_deriv_from_output(h) - dref).max() <= nr.DERIV_BAR, (nr.LAYER_NAMES[kind], W)


def test_numerics_probe_cross_compiles_for_gfx950():
    """The probe builds with the product's own compiler and flags (one fragment, csrc/flags.mk) and exports its entry
    points; it is not part of libcude_hip.so."""
    import ctypes
    import numerics_ref as nr
    csrc = os.path.join(ROOT, "conditional-ude_amd", "csrc")
    probe_cmd = subprocess.check_output(["make", "-n", "-B", "-C", nr.HIP_DIR, "libnumerics_probe.so"]).decode()
    lib_cmd = subprocess.check_output(["make", "-n", "-B", "-C", csrc, "cude_common.o"]).decode()
    flags = [ln for ln in lib_cmd.splitlines() if "cude_common.hip" in ln][0].split(" -c ")[0]
    assert "--offload-arch=gfx950" in flags and flags in probe_cmd, (flags, probe_cmd)
    assert " -D" not in probe_cmd
    nr.build("libnumerics_probe.so", timeout=300)
    lib = ctypes.CDLL(os.path.join(nr.HIP_DIR, "libnumerics_probe.so"))
    for sym in ("probe_elementwise", "probe_tanh_table", "probe_layer", "probe_net_info", "probe_net",
                "probe_param_check"):
        assert hasattr(lib, sym), sym
    product = open(os.path.join(csrc, "libcude_hip.so"), "rb").read() if os.path.exists(
        os.path.join(csrc, "libcude_hip.so")) else b""
    assert b"probe_elementwise" not in product
