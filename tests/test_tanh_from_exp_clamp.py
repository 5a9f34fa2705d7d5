"""m_tanh_from_exp (csrc/cude_math.h) clamps the denominator E + 1 behind the add; it used to clamp E in front of it.
The two forms are the same function of E, bit for bit: the cap is e^40, where one ulp is 32, so cap + 1 == cap; below
the cap rounding is monotone; above it, for +Inf and for NaN both give the cap.  A host program carries the former
expression inline and compares the header's function with it for the widths that have a layer-1 exponent table (6 and
7) on vectors that mix ordinary values with the cap's neighbourhood and with the values that only a clamp makes
harmless, each of those in every position of the vector."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "cude_math.h"
#include <cstdio>
#include <cstring>
#include <cmath>
#include <cstdint>
#include <limits>
#include <random>
#include <vector>
// the expression this function had before the clamp moved: min(E, e^40) + 1
template <int W>
static void reference(const double (&E)[W], double (&t)[W]) {
  double d[W], pre[W];
  for (int j = 0; j < W; j++) d[j] = fmin(E[j], 2.35385266837019985408e17) + 1.0;
  pre[0] = d[0];
  for (int j = 1; j < W; j++) pre[j] = pre[j - 1] * d[j];
  double r = cude::m_rcp(pre[W - 1]);
  for (int j = W - 1; j >= 1; j--) {
    const double inv = r * pre[j - 1];
    r = r * d[j];
    t[j] = fma(-2.0, inv, 1.0);
  }
  t[0] = fma(-2.0, r, 1.0);
}
static long n_vec = 0, n_bad = 0, n_nonfinite = 0;
template <int W>
static void compare(const double (&E)[W]) {
  double a[W], b[W];
  cude::m_tanh_from_exp<W>(E, a);
  reference<W>(E, b);
  n_vec++;
  if (std::memcmp(a, b, sizeof a) != 0) n_bad++;
  for (int j = 0; j < W; j++) if (!std::isfinite(a[j])) n_nonfinite++;
}
template <int W>
static void run(const std::vector<double>& special) {
  std::mt19937_64 g(7 + W);
  std::uniform_real_distribution<double> U(-1, 1);
  double E[W];
  // ordinary values: exp(2 z), z up to +-25 (both sides of the clamp at z = 20) and up to +-350 (the table's range)
  for (int i = 0; i < 200000; i++) {
    const double s = (i & 1) ? 25.0 : 350.0;
    for (int j = 0; j < W; j++) E[j] = std::exp(2.0 * s * U(g));
    compare<W>(E);
  }
  // every special value in every position, the other positions ordinary; then two and all positions special
  for (double v : special)
    for (int k = 0; k < W; k++)
      for (int rep = 0; rep < 8; rep++) {
        for (int j = 0; j < W; j++) E[j] = std::exp(2.0 * 12.0 * U(g));
        E[k] = v;
        compare<W>(E);
        E[(k + 1 + rep % (W - 1)) % W] = special[(size_t)(g() % special.size())];
        compare<W>(E);
      }
  for (double v : special) {
    for (int j = 0; j < W; j++) E[j] = v;
    compare<W>(E);
  }
}
int main() {
  const double cap = 2.35385266837019985408e17;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> special = {
      0.0, std::numeric_limits<double>::denorm_min(), 2.5e-310, std::numeric_limits<double>::min(),
      cap, std::nextafter(cap, 0.0), std::nextafter(cap, inf), cap - 15.0, cap - 16.0, cap - 17.0, cap - 32.0, cap - 48.0,
      cap + 64.0, 9007199254740992.0 /* 2^53: E + 1 rounds */, 9007199254740993.0, 9007199254740994.0, 1.0, 1e300,
      std::numeric_limits<double>::max(), inf, std::numeric_limits<double>::quiet_NaN()};
  run<6>(special);
  run<7>(special);
  printf("%ld %ld %ld\n", n_vec, n_bad, n_nonfinite);
  return 0;
}
'''


def test_clamp_behind_the_add_gives_the_bits_of_the_clamp_in_front_of_it():
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(SRC)
        exe = os.path.join(d, "t")
        # -ffp-contract=off: the reference's min(E, cap) + 1 and the products must not be fused differently in the two
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "conditional-ude_amd", "csrc"),
                               os.path.join(d, "t.cpp"), "-o", exe])
        n_vec, n_bad, n_nonfinite = (int(v) for v in subprocess.check_output([exe]).decode().split())
    assert n_vec > 400000
    assert n_bad == 0, f"{n_bad} of {n_vec} vectors differ"
    assert n_nonfinite == 0          # the clamp's purpose: +Inf and NaN among the exponentials give tanh = 1, not NaN
