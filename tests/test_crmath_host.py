"""csrc/crmath.h on the host: the header's sin, cos, tan, asin, acos and atan2 (the functions
reeds_shepp.hip rounds as glibc does) compiled as plain C++ and compared with the long double libm rounded
to double.

Bounds.  A result may differ from that reference by one ulp at most.  The reference itself is not the
correctly rounded double everywhere: a long double carries 11 bits more than a double, and rounding its
last-bit-uncertain value a second time goes the other way for about 2^-11 = 0.05 % of arguments, so the
share of differing results must stay below 0.1 %; the host's own double libm, which is not correctly rounded
either, is printed beside it."""
import shutil
import subprocess

import pytest

from golden_io import GOLDEN

SRC = r"""
#define CRM_FN static inline
#include "crmath.h"
#include <cstdio>
#include <cstring>
#include <random>
static long ulps(double a, double b)
{
    long long x, y;
    memcpy(&x, &a, 8);
    memcpy(&y, &b, 8);
    if (x < 0) x = (long long)0x8000000000000000ULL - x;
    if (y < 0) y = (long long)0x8000000000000000ULL - y;
    return (long)llabs(x - y);
}
int main()
{
    std::mt19937_64 g(1);
    std::uniform_real_distribution<double> U(-70, 70), V(-1, 1), W(-40, 40);
    const int N = 200000;
    long mis[6] = {0}, worst[6] = {0}, host[6] = {0};
    for (int i = 0; i < N; i++) {
        double x = U(g), v = V(g), a = W(g), b = W(g);
        if (i % 4 == 0) { x *= 1e-3; a *= 1e-6; }                           // small angles
        if (i % 7 == 0) v = (v > 0 ? 1 : -1) * (1 - 1e-9 * fabs(V(g)));     // the ends of asin / acos
        const double r[6] = {crm::sin(x), crm::cos(x), crm::tan(x), crm::asin(v), crm::acos(v), crm::atan2(a, b)};
        const double e[6] = {(double)sinl(x), (double)cosl(x), (double)tanl(x), (double)asinl(v), (double)acosl(v),
                             (double)atan2l(a, b)};
        const double h[6] = {sin(x), cos(x), tan(x), asin(v), acos(v), atan2(a, b)};
        for (int j = 0; j < 6; j++) {
            const long d = ulps(r[j], e[j]);
            if (d) mis[j]++;
            if (d > worst[j]) worst[j] = d;
            if (h[j] != e[j]) host[j]++;
        }
    }
    for (int j = 0; j < 6; j++) printf("%ld %ld %ld\n", mis[j], worst[j], host[j]);
    // signed zeros and the exact values stay the libm's
    printf("%d\n", std::signbit(crm::sin(-0.0)) && crm::cos(0.0) == 1.0 && crm::atan2(0.0, -0.0) == atan2(0.0, -0.0) &&
                       crm::atan2(0.0, 0.0) == 0.0 && crm::asin(1.0) == asin(1.0) && crm::acos(-1.0) == acos(-1.0) &&
                       crm::atan2(1.0, 0.0) == atan2(1.0, 0.0) && std::isnan(crm::atan2(NAN, 1.0)) && std::isnan(crm::sin(NAN)));
    return 0;
}
"""


def test_header_rounds_as_the_long_double_libm(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    import os

    csrc = os.path.join(os.path.dirname(GOLDEN), "..", "python_motion_planning_amd", "csrc")
    (tmp_path / "t.cpp").write_text(SRC)
    exe = str(tmp_path / "t")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", csrc, "-o", exe, str(tmp_path / "t.cpp"), "-lm"])
    out = subprocess.check_output([exe], text=True).split("\n")
    names = ("sin", "cos", "tan", "asin", "acos", "atan2")
    rows = [tuple(int(v) for v in ln.split()) for ln in out[:6]]
    print({n: dict(differ=r[0], worst_ulp=r[1], host_libm_differs=r[2]) for n, r in zip(names, rows)}, "of 200000")
    for n, (mis, worst, _) in zip(names, rows):
        assert worst <= 1, (n, worst)
        assert mis <= 200, (n, mis)  # 0.1 % of 200,000
    assert out[6].strip() == "1"
