"""The clamp-free activations of csrc/cude_math.h and the test that licenses them (m_lean_bounds), on the host.

The fixed-step c-peptide gradient kernel drops min(|z|, 20) from the tanh layers above the first and max(-0.5 |x|, -350)
from the output unit's softplus where the parameter set proves |z| <= 19.5 and |x| <= 690 (csrc/cude_cpep.hip).  Under
those bounds a clamp returns its argument, so the clamp-free form must be the clamped one BIT FOR BIT.  A host program
compares the two forms of m_tanh_vec for the widths that have them (6 and 7) and of m_softplus_t (both Horner variants)
on random arguments inside the bounds and on the neighbourhood of the bounds and of the clamps themselves, in every
position of the vector; up to the clamp's own threshold, inclusive, the forms agree, and one probe beyond it shows that the
comparison sees a clamp that acts.  The bound function is probed with rows that sum to exactly the threshold, to its
neighbours on either side, and with NaN / Inf in every entry it reads: those come out "not lean"."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "cude_math.h"
#include <cstdio>
#include <cstring>
#include <cmath>
#include <limits>
#include <random>
#include <vector>
static long n_vec = 0, n_bad = 0, n_sp = 0, n_sp_bad = 0, n_flag = 0, n_flag_bad = 0, n_setup_bad = 0, n_seen = 0;
template <int W>
static void compare(const double (&z)[W]) {
  double a[W], b[W];
  cude::m_tanh_vec<W, true>(z, a);
  cude::m_tanh_vec<W, false>(z, b);
  n_vec++;
  if (std::memcmp(a, b, sizeof a) != 0) n_bad++;
}
template <int W>
static void run_tanh() {
  std::mt19937_64 g(11 + W);
  std::uniform_real_distribution<double> U(-1, 1);
  const double inf = std::numeric_limits<double>::infinity();
  double z[W];
  for (int i = 0; i < 200000; i++) {
    const double s = (i % 3 == 0) ? 19.5 : (i % 3 == 1) ? 3.0 : 0.05;      // the whole range, the usual one, near zero
    for (int j = 0; j < W; j++) z[j] = s * U(g);
    compare<W>(z);
  }
  // the bound, the clamp's threshold (where min returns either argument: the same number) and their neighbours
  std::vector<double> edge = {19.5, std::nextafter(19.5, 0.0), std::nextafter(19.5, inf), 19.4, 19.6, 19.999999,
                              std::nextafter(20.0, 0.0), 20.0, 0.0, std::numeric_limits<double>::denorm_min(), 1e-300};
  for (double v : edge)
    for (int sgn = -1; sgn <= 1; sgn += 2)
      for (int k = 0; k < W; k++)
        for (int rep = 0; rep < 8; rep++) {
          for (int j = 0; j < W; j++) z[j] = 19.5 * U(g);
          z[k] = sgn * v;
          compare<W>(z);
          z[(k + 1 + rep % (W - 1)) % W] = -sgn * edge[(size_t)(g() % edge.size())];
          compare<W>(z);
        }
  for (double v : edge) {
    for (int j = 0; j < W; j++) z[j] = (j & 1) ? v : -v;
    compare<W>(z);
  }
}
template <bool LONE>
static void compare_sp(double x) {
  double sa, sb;
  const double a = cude::m_softplus_t<LONE, true>(x, &sa);
  const double b = cude::m_softplus_t<LONE, false>(x, &sb);
  n_sp++;
  if (std::memcmp(&a, &b, 8) != 0 || std::memcmp(&sa, &sb, 8) != 0) n_sp_bad++;
}
static void run_softplus() {
  std::mt19937_64 g(5);
  std::uniform_real_distribution<double> U(-1, 1);
  const double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < 200000; i++) {
    const double s = (i % 3 == 0) ? 690.0 : (i % 3 == 1) ? 30.0 : 2.0;
    const double x = s * U(g);
    compare_sp<false>(x);
    compare_sp<true>(x);
  }
  for (double v : {690.0, std::nextafter(690.0, 0.0), std::nextafter(690.0, inf), 689.0, 691.0, 699.999,
                   std::nextafter(700.0, 0.0), 700.0, 0.0, 1e-300})
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      compare_sp<false>(sgn * v);
      compare_sp<true>(sgn * v);
    }
}
// beyond the thresholds the forms are different functions, and the comparisons above would show it
static void run_seen() {
  const double a = cude::m_tanh_den_t<true>(25.0), b = cude::m_tanh_den_t<false>(25.0);
  if (a != b && b == cude::m_tanh_den_t<false>(20.0)) n_seen++;
  double sa, sb;
  cude::m_softplus_t<false, true>(-720.0, &sa);
  cude::m_softplus_t<false, false>(-720.0, &sb);
  if (sa != sb) n_seen++;
}
// ---- the bound function.  Layout: [W1 (w x nin); b1 (w)] then per further hidden layer [W (w x w, column-major); b (w)],
// then [w_out (w); b_out]
struct Net { int nin, w, d; };
static int n_par(const Net& n) { return n.w * n.nin + n.w + (n.d - 1) * (n.w * n.w + n.w) + n.w + 1; }
static void expect(const std::vector<double>& p, const Net& n, bool tanh_lean, bool out_lean) {
  bool t = !tanh_lean, o = !out_lean;
  cude::m_lean_bounds(p.data(), n.nin, n.w, n.d, &t, &o);
  n_flag++;
  if (t != tanh_lean || o != out_lean) n_flag_bad++;
}
// row j of hidden layer l (1-based above the first) with |b| + sum |W| == target (exact: to the bit, in the order the bound
// function adds): weights a with alternating signs
static void set_row(std::vector<double>& p, const Net& n, int l, int j, double a, double target, bool exact = true) {
  const int o = n.w * n.nin + n.w + (l - 1) * (n.w * n.w + n.w);
  double s = std::fabs(target - n.w * a);
  p[o + n.w * n.w + j] = (j & 1) ? s : -s;
  for (int k = 0; k < n.w; k++) {
    p[o + n.w * k + j] = (k & 1) ? -a : a;
    s += a;
  }
  if (exact && s != target) n_setup_bad++;
}
static void set_out(std::vector<double>& p, const Net& n, double a, double target, bool exact = true) {
  const int o = n_par(n) - n.w - 1;
  double s = std::fabs(target - n.w * a);
  p[o + n.w] = -s;
  for (int k = 0; k < n.w; k++) {
    p[o + k] = (k & 1) ? a : -a;
    s += a;
  }
  if (exact && s != target) n_setup_bad++;
}
static void run_bounds() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::mt19937_64 g(3);
  std::uniform_real_distribution<double> U(-1, 1);
  for (Net n : {Net{2, 6, 2}, Net{2, 7, 2}, Net{3, 6, 2}, Net{2, 6, 3}, Net{2, 7, 3}, Net{2, 6, 1}}) {
    std::vector<double> base((size_t)n_par(n));
    for (double& v : base) v = U(g);                               // rows sum to at most w + 1 <= 8
    for (int q = 0; q < n.w * n.nin + n.w; q++) base[(size_t)q] *= 1e6;   // layer 1 is no part of the test
    expect(base, n, true, true);
    const int first_upper = n.w * n.nin + n.w;
    for (int l = 1; l < n.d; l++)
      for (int j = 0; j < n.w; j++) {
        std::vector<double> p = base;
        set_row(p, n, l, j, 2.0, 19.5);                            expect(p, n, true, true);
        set_row(p, n, l, j, 2.0, std::nextafter(19.5, 0.0));       expect(p, n, true, true);
        set_row(p, n, l, j, 2.0, std::nextafter(19.5, inf));       expect(p, n, false, true);
        set_row(p, n, l, j, 2.0, 19.4, false);                     expect(p, n, true, true);
        set_row(p, n, l, j, 2.0, 19.6, false);                     expect(p, n, false, true);
        set_row(p, n, l, j, 8.0, 60.0);                            expect(p, n, false, true);
      }
    {
      std::vector<double> p = base;
      set_out(p, n, 64.0, 690.0);                                  expect(p, n, true, true);
      set_out(p, n, 64.0, std::nextafter(690.0, 0.0));             expect(p, n, true, true);
      set_out(p, n, 64.0, std::nextafter(690.0, inf));             expect(p, n, true, false);
      set_out(p, n, 64.0, 800.0, false);                           expect(p, n, true, false);
      set_out(p, n, 1e300, 1.5e301, false);                        expect(p, n, true, false);
    }
    // a non-finite entry anywhere above the first layer: its flag is false (both signs of Inf, NaN)
    for (int q = first_upper; q < n_par(n); q++)
      for (double bad : {nan, inf, -inf}) {
        std::vector<double> p = base;
        p[(size_t)q] = bad;
        const bool in_out = q >= n_par(n) - n.w - 1;
        expect(p, n, in_out, !in_out);
      }
    // ... and in the first layer: none of this test's business (the kernel's parameter check reports it)
    for (int q = 0; q < first_upper; q++) {
      std::vector<double> p = base;
      p[(size_t)q] = nan;
      expect(p, n, true, true);
    }
  }
}
int main() {
  run_tanh<6>();
  run_tanh<7>();
  run_softplus();
  run_seen();
  run_bounds();
  printf("%ld %ld %ld %ld %ld %ld %ld %ld\n", n_vec, n_bad, n_sp, n_sp_bad, n_flag, n_flag_bad, n_setup_bad, n_seen);
  return 0;
}
'''


def test_clamp_free_forms_have_the_bits_of_the_clamped_ones_inside_the_bounds():
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(SRC)
        exe = os.path.join(d, "t")
        # -ffp-contract=off: both forms must be compiled to the same operations around the clamp
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I",
                               os.path.join(ROOT, "conditional-ude_amd", "csrc"), os.path.join(d, "t.cpp"), "-o", exe])
        n_vec, n_bad, n_sp, n_sp_bad, n_flag, n_flag_bad, n_setup_bad, n_seen = (
            int(v) for v in subprocess.check_output([exe]).decode().split())
    assert n_vec > 400000 and n_sp > 400000 and n_flag > 500
    assert n_bad == 0, f"tanh: {n_bad} of {n_vec} vectors differ"
    assert n_sp_bad == 0, f"softplus: {n_sp_bad} of {n_sp} arguments differ"
    assert n_setup_bad == 0            # the probes' rows sum to exactly what they were built for
    assert n_flag_bad == 0, f"bound function: {n_flag_bad} of {n_flag} probes misjudged"
    assert n_seen == 2                 # beyond its threshold either clamp changes the result: the comparison sees clamps
