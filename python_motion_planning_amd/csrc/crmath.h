// sin, cos, tan, asin, acos and atan2 rounded as the exact value rounds (up to a double-double error of
// about 2^-70: the result is the correctly rounded one unless the exact value lies that close to the middle
// of two doubles).  The device's libm is within an ulp of glibc's but not bit-equal; glibc's own results
// are the correctly rounded ones in all but about one call in a thousand.  Where the reference decides on
// an exact comparison of a value that is 0 mathematically (the strip of trailing points whose local x is
// exactly 0.0, curve_generation/reeds_shepp.py:664-667), an ulp in any of these calls changes the answer,
// so reeds_shepp.hip computes them here.
//  - sincos_dd: Cody-Waite reduction by pi/2 in four parts (exact products for |k| < 2^20), then the
//    Taylor series of sin and cos on |r| <= pi/4 + in double-double (the leading terms) and double (the
//    tail, which contributes less than 2^-20 of the result);
//  - the inverse functions: the device's result a0, then one Newton step with sincos_dd(a0), whose
//    cancelling numerator is formed from error-free products.
// Arguments beyond 1e5 in magnitude go to the device's libm (reeds_shepp.hip bounds its angles at 64).
#pragma once
#include <cmath>
#ifndef CRM_FN
#define CRM_FN __device__ __forceinline__
#endif

namespace crm {

struct dd {
    double h, l;
};

CRM_FN dd two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return dd{s, (a - (s - bb)) + (b - bb)};
}
CRM_FN dd fast_two_sum(double a, double b)  // |a| >= |b|
{
    const double s = a + b;
    return dd{s, b - (s - a)};
}
CRM_FN dd two_prod(double a, double b)
{
    const double p = a * b;
    return dd{p, fma(a, b, -p)};
}
CRM_FN dd add(dd a, dd b)
{
    dd s = two_sum(a.h, b.h);
    const dd t = two_sum(a.l, b.l);
    s.l += t.h;
    s = fast_two_sum(s.h, s.l);
    s.l += t.l;
    return fast_two_sum(s.h, s.l);
}
CRM_FN dd mul(dd a, dd b)
{
    dd p = two_prod(a.h, b.h);
    p.l += a.h * b.l + a.l * b.h;
    return fast_two_sum(p.h, p.l);
}
CRM_FN dd neg(dd a) { return dd{-a.h, -a.l}; }

// sin(x) and cos(x) as double-doubles, 0 < |x| <= 1e5
CRM_FN void sincos_dd(double x, dd& s, dd& c)
{
    // pi/2 = P1 + P2 + P3 + P3T, the first three of 33 bits each (fdlibm's e_rem_pio2.c)
    const double P1 = 1.57079632673412561417e+00, P2 = 6.07710050630396597660e-11, P3 = 2.02226624871116645580e-21,
                 P3T = 8.47842766036889956997e-32;
    const double k = rint(x * 6.36619772367581382433e-01);
    dd r = two_sum(x - k * P1, -(k * P2));  // x - k P1 is exact (Sterbenz), as are the products
    const dd t = two_sum(r.h, -(k * P3));
    r = fast_two_sum(t.h, (r.l + t.l) - k * P3T);
    const dd r2 = mul(r, r);
    const double z = r2.h;
    // sin r = r + r r2 (S3 + r2 (S5 + r2 (S7 + r2 (S9 + r2 Qs)))), (-1)^j / (2j + 1)!
    const double qs = -2.505210838544172e-08 + z * (1.6059043836821613e-10 + z * (-7.647163731819816e-13 + z * (2.8114572543455206e-15 + z * (-8.22063524662433e-18 + z * (1.9572941063391263e-20 + z * -3.868170170630684e-23)))));
    dd u = add(mul(dd{qs, 0.0}, r2), dd{2.7557319223985893e-06, -1.858393274046472e-22});
    u = add(mul(u, r2), dd{-0.0001984126984126984, -1.7209558293420705e-22});
    u = add(mul(u, r2), dd{0.008333333333333333, 1.1564823173178714e-19});
    u = add(mul(u, r2), dd{-0.16666666666666666, -9.25185853854297e-18});
    dd sr = add(r, mul(r, mul(u, r2)));
    // cos r = 1 + r2 (C2 + r2 (C4 + r2 (C6 + r2 (C8 + r2 (C10 + r2 Qc))))), (-1)^j / (2j)!
    const double qc = 2.08767569878681e-09 + z * (-1.1470745597729725e-11 + z * (4.779477332387385e-14 + z * (-1.5619206968586225e-16 + z * (4.110317623312165e-19 + z * (-8.896791392450574e-22 + z * 1.6117375710961184e-24)))));
    dd v = add(mul(dd{qc, 0.0}, r2), dd{-2.755731922398589e-07, -2.3767714622250297e-23});
    v = add(mul(v, r2), dd{2.48015873015873e-05, 2.1511947866775882e-23});
    v = add(mul(v, r2), dd{-0.001388888888888889, 5.300543954373577e-20});
    v = add(mul(v, r2), dd{0.041666666666666664, 2.3129646346357427e-18});
    v = add(mul(v, r2), dd{-0.5, 0.0});
    dd cr = add(dd{1.0, 0.0}, mul(v, r2));
    switch ((long long)k & 3) {
        case 0: s = sr; c = cr; break;
        case 1: s = cr; c = neg(sr); break;
        case 2: s = neg(sr); c = neg(cr); break;
        default: s = neg(cr); c = sr; break;
    }
}

CRM_FN bool in_range(double x) { return fabs(x) <= 1e5; }  // false for a NaN

CRM_FN double sin(double x)
{
    if (!in_range(x)) return ::sin(x);
    if (x == 0.0) return x;
    dd s, c;
    sincos_dd(x, s, c);
    return s.h;
}
CRM_FN double cos(double x)
{
    if (!in_range(x)) return ::cos(x);
    if (x == 0.0) return 1.0;
    dd s, c;
    sincos_dd(x, s, c);
    return c.h;
}
// both at once: the same bits as sin(x) and cos(x)
CRM_FN void sincos(double x, double& sn, double& cs)
{
    if (!in_range(x) || x == 0.0) {
        sn = crm::sin(x);
        cs = crm::cos(x);
        return;
    }
    dd s, c;
    sincos_dd(x, s, c);
    sn = s.h;
    cs = c.h;
}
CRM_FN double tan(double x)
{
    if (!in_range(x)) return ::tan(x);
    if (x == 0.0) return x;
    dd s, c;
    sincos_dd(x, s, c);
    const double q = s.h / c.h;
    const dd p = two_prod(q, c.h);
    const double rem = ((s.h - p.h) - p.l) + (s.l - q * c.l);
    return q + rem / c.h;
}
// asin on [-1, 1]: a0, then a0 + (x - sin a0) / cos a0
CRM_FN double asin(double x)
{
    const double a0 = ::asin(x);
    if (!(fabs(x) < 1.0) || x == 0.0) return a0;  // the ends are exact; NaN
    dd s, c;
    sincos_dd(a0, s, c);
    return a0 + (((x - s.h) - s.l) / c.h);
}
// acos on [-1, 1]: a0, then a0 + (cos a0 - x) / sin a0
CRM_FN double acos(double x)
{
    const double a0 = ::acos(x);
    if (!(fabs(x) < 1.0)) return a0;
    dd s, c;
    sincos_dd(a0, s, c);
    return a0 + (((c.h - x) + c.l) / s.h);
}
// atan2: a0, then a0 + (y cos a0 - x sin a0) / (x cos a0 + y sin a0)
CRM_FN double atan2(double y, double x)
{
    const double a0 = ::atan2(y, x);
    const double m = fmax(fabs(x), fabs(y));
    // zeros, infinities and NaNs have exact results; a0 == 0 only when the quotient underflows
    if (x == 0.0 || y == 0.0 || a0 != a0 || !(m < __builtin_huge_val()) || a0 == 0.0 || !(m < 1e150) || !(m > 1e-150)) return a0;
    dd s, c;
    sincos_dd(a0, s, c);
    const dd yc = two_prod(y, c.h), xs = two_prod(x, s.h);
    const double num = ((yc.h - xs.h) + (yc.l - xs.l)) + (y * c.l - x * s.l);
    const double den = x * c.h + y * s.h;
    return a0 + num / den;
}

}  // namespace crm
