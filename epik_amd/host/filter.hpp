// filter.hpp -- the rule of ranking phylo-k-mers by informativeness (include/epik_amd.h, "Ranking phylo-k-mers by
// informativeness"): ek_exp2 and ek_log2, the terms of an entry, the value of a key from its sums and the sortable
// image of a value, as functions that the kernels (csrc/filter_place.hip) and the host mirror (filter.cpp) share word
// for word; and what epik_amd_filter_rank_host and epik_amd_filter_math_host run.  Plain C++; under hipcc the inline
// functions are __host__ __device__.  Every translation unit that includes it is compiled with -ffp-contract=off.
#ifndef EPIK_AMD_HOST_FILTER_HPP
#define EPIK_AMD_HOST_FILTER_HPP
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "epik_amd.h"

#if defined(__HIPCC__)
#define EK_HD __host__ __device__
#else
#define EK_HD
#endif

namespace epik_amd {

constexpr uint32_t kFilterChains = 64;
constexpr double kLog2Of10 = 3.321928094887362;      // 0x1.a934f0979a371p+1
constexpr double kLn2 = 0.6931471805599453;          // 0x1.62e42fefa39efp-1
constexpr double kTwoOverLn2 = 2.8853900817779268;   // 0x1.71547652b82fep+1
constexpr double kSqrtHalf = 0.7071067811865476;     // 0x1.6a09e667f3bcdp-1

// 2^x for x <= 1023 (the rule calls it with x <= 0): +0.0 below -1022, so that no result is subnormal and ldexp is exact
EK_HD inline double ek_exp2(double x)
{
    if (!(x >= -1022.0)) return 0.0;  // (-inf as well; the rule never passes a NaN)
    if (x > 1023.0) return HUGE_VAL;
    const double n = rint(x);  // ties to even
    const double r = x - n;    // exact, |r| <= 0.5
    const double y = r * kLn2;
    double q = 1.6059043836821613e-10;  // 1/13!
    q = q * y + 2.08767569878681e-09;   // 1/12!
    q = q * y + 2.505210838544172e-08;
    q = q * y + 2.755731922398589e-07;
    q = q * y + 2.7557319223985893e-06;
    q = q * y + 2.48015873015873e-05;
    q = q * y + 0.0001984126984126984;
    q = q * y + 0.001388888888888889;
    q = q * y + 0.008333333333333333;
    q = q * y + 0.041666666666666664;
    q = q * y + 0.16666666666666666;
    q = q * y + 0.5;
    q = q * y + 1.0;
    q = q * y + 1.0;
    return ldexp(q, (int)n);
}

// log2 z for a finite z > 0; -inf at 0, +inf at +inf, NaN below 0 (the rule passes finite z > 0 only)
EK_HD inline double ek_log2(double z)
{
    if (!(z > 0.0)) return z == 0.0 ? -HUGE_VAL : NAN;
    if (z == HUGE_VAL) return z;
    int e = 0;
    double m = frexp(z, &e);  // [0.5, 1)
    if (m < kSqrtHalf) m = m * 2.0, e -= 1;  // [sqrt 1/2, sqrt 2)
    const double t = (m - 1.0) / (m + 1.0);
    const double u = t * t;
    double q = 0.043478260869565216;  // 1/23
    q = q * u + 0.047619047619047616;
    q = q * u + 0.05263157894736842;
    q = q * u + 0.058823529411764705;
    q = q * u + 0.06666666666666667;
    q = q * u + 0.07692307692307693;
    q = q * u + 0.09090909090909091;
    q = q * u + 0.1111111111111111;
    q = q * u + 0.14285714285714285;
    q = q * u + 0.2;
    q = q * u + 0.3333333333333333;
    q = q * u + 1.0;
    return (double)e + (t * q) * kTwoOverLn2;
}

// the two terms of an entry of score s: p = 2^x and p x, the second +0.0 where p is 0 (x may be -inf)
EK_HD inline void filter_terms(float s, double &p, double &px)
{
    const double x = (double)s * kLog2Of10;
    p = ek_exp2(x);
    px = p == 0.0 ? 0.0 : p * x;
}

// mif0 of a list of n entries whose terms sum to A and B
EK_HD inline double filter_mif0(double A, double B, uint64_t n, uint32_t num_branches, float log_thr)
{
    const double xt = (double)log_thr * kLog2Of10;
    const double t = ek_exp2(xt);
    const double missing = n < num_branches ? (double)(num_branches - n) : 0.0;
    const double R = missing * t;
    const double C = R == 0.0 ? 0.0 : R * xt;
    const double Z = A + R;
    if (Z == 0.0) return HUGE_VAL;
    return ek_log2(Z) - ((B + C) / Z);
}

// best: minus the largest score of the list (+inf for an empty list)
EK_HD inline double filter_best(float max_score, uint64_t n) { return n ? -(double)max_score : HUGE_VAL; }

// random: the top 53 bits of the splitmix64 finaliser of seed + key * 0x9E3779B97F4A7C15
EK_HD inline double filter_random(uint64_t seed, uint32_t key)
{
    uint64_t z = seed + (uint64_t)key * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11);
}

// -0.0 counts as +0.0
EK_HD inline double filter_fold_zero(double v) { return v == 0.0 ? 0.0 : v; }

// a uint64 that orders as the (folded, never NaN) double does
EK_HD inline uint64_t filter_image(double v)
{
    uint64_t bits;
    memcpy(&bits, &v, sizeof bits);
    return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;
}

// what can be refused before the arrays are looked at
int filter_check_params(uint32_t num_branches, float log_thr, uint32_t filter, std::string &err);
// the messages of the three refusals that name an offender (the device finds them in a kernel)
std::string filter_bad_offsets(uint64_t k, uint64_t lo, uint64_t hi, uint64_t total);
std::string filter_bad_score(uint64_t i, float score);
std::string filter_bad_branch(uint64_t i, uint32_t branch, uint32_t num_branches);

// the rule on `num_threads` threads (0: one): value [K] and order [K]; EPIK_AMD_ERR_INVALID with `err` for the refusals
int filter_rank_host(uint32_t num_branches, float log_thr, const uint32_t *keys, const uint64_t *offsets,
                     const epik_amd_pkdb_value *values, uint64_t K, uint32_t filter, uint64_t seed, uint32_t num_threads,
                     double *value, uint32_t *order, std::string &err);

// exp2_out[i] = ek_exp2(x[i]), log2_out[i] = ek_log2(x[i]); either output may be null
void filter_math_host(const double *x, uint64_t n, double *exp2_out, double *log2_out);

}  // namespace epik_amd
#endif
