// Shortest round-trip decimal text of a float, as CPython's repr(float(v)) writes it, in integer arithmetic only -- shared by
// the kernels of text.hip and by host code (the functions compile for both).
//
// The value is widened to double first (exactly), so the digits are the shortest string that reads back as that DOUBLE, the
// closest to it among the shortest, an exact tie going to the even digit: Steele & White's free-format generation (dragon4)
// on multi-word integers.  With v = M 2^E (M of 53 bits), the state is
//     r / s = v,   mm / s = half the gap to the double below,   mp / s = half the gap above (= mm, or 2 mm when M = 2^52)
// scaled by a power of ten so that 1/10 <= v' < 1, and every digit is d = floor(10 r / s), r <- 10 r - d s, until the rest
// lies within the gaps.  Numbers are NL words of 32 bits in registers (every loop is unrolled over constant word indices):
// 4 words hold the state for 2^-66 <= |v| < 2^111, 8 words hold every float (the smallest subnormal needs s = 2^203; a
// host build can count every carry out of the top word, and the tests do).  The quotient digit is ESTIMATED in double (r and s rounded to double, one multiply by 1 / s) from below
// and corrected by one exact compare-and-subtract, so no result depends on floating-point rounding.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define CPC_TEXT_HD __host__ __device__ __forceinline__
#else
#define CPC_TEXT_HD inline
#endif
#ifndef CPC_TEXT_CHECK          // (host test builds define it as an assert on the carries that must be zero)
#define CPC_TEXT_CHECK(cond) ((void)0)
#endif

namespace cpc {
namespace text {

constexpr int SLOT_BYTES = 24;       // the longest texts have 23 bytes: -1.1754943508222875e-38, -0.00012345678901234567

template <int NL> struct Big { uint32_t w[NL]; };

// a = v << sh  (v != 0, 0 <= sh)
template <int NL> CPC_TEXT_HD void big_set(Big<NL> &a, uint64_t v, int sh)
{
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int lo = 32 * i - sh;                     // bit of v that lands on bit 0 of word i
        uint32_t word = 0;
        if (lo >= 0 && lo < 64) word = (uint32_t)(v >> lo);
        else if (lo < 0 && lo > -32) word = (uint32_t)(v << -lo);
        a.w[i] = word;
    }
    CPC_TEXT_CHECK(v != 0 && sh + 64 - __builtin_clzll(v) <= 32 * NL);
}
template <int NL> CPC_TEXT_HD void big_mul(Big<NL> &a, uint32_t m)
{
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const uint64_t p = (uint64_t)a.w[i] * m + carry;
        a.w[i] = (uint32_t)p;
        carry = p >> 32;
    }
    CPC_TEXT_CHECK(carry == 0);
}
template <int NL> CPC_TEXT_HD void big_mul_pow10(Big<NL> &a, int n)
{
    for (; n >= 9; n -= 9) big_mul(a, 1000000000u);
    uint32_t m = 1;
    for (int j = 0; j < n; ++j) m *= 10u;
    if (n > 0) big_mul(a, m);
}
template <int NL> CPC_TEXT_HD void big_add(Big<NL> &a, const Big<NL> &b)
{
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const uint64_t t = (uint64_t)a.w[i] + b.w[i] + carry;
        a.w[i] = (uint32_t)t;
        carry = t >> 32;
    }
    CPC_TEXT_CHECK(carry == 0);
}
template <int NL> CPC_TEXT_HD void big_sub(Big<NL> &a, const Big<NL> &b)            // a >= b
{
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const uint64_t t = (uint64_t)a.w[i] - b.w[i] - borrow;
        a.w[i] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
    CPC_TEXT_CHECK(borrow == 0);
}
// a -= q * b  (q * b <= a)
template <int NL> CPC_TEXT_HD void big_submul(Big<NL> &a, const Big<NL> &b, uint32_t q)
{
    uint64_t carry = 0, borrow = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const uint64_t p = (uint64_t)b.w[i] * q + carry;
        carry = p >> 32;
        const uint64_t t = (uint64_t)a.w[i] - (uint32_t)p - borrow;
        a.w[i] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
    CPC_TEXT_CHECK(carry == 0 && borrow == 0);
}
template <int NL> CPC_TEXT_HD int big_cmp(const Big<NL> &a, const Big<NL> &b)        // -1, 0, +1
{
    int res = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i)                        // (the highest differing word decides: it is visited last)
        if (a.w[i] != b.w[i]) res = a.w[i] < b.w[i] ? -1 : 1;
    return res;
}
template <int NL> CPC_TEXT_HD double big_to_double(const Big<NL> &a)
{
    double d = 0.0;
#pragma unroll
    for (int i = NL - 1; i >= 0; --i) d = d * 4294967296.0 + (double)a.w[i];
    return d;
}

// is v + (the gap above) beyond s, i.e. does the interval of strings that read back as v reach 1?
template <int NL> CPC_TEXT_HD bool reaches(const Big<NL> &r, const Big<NL> &mm, bool twice, const Big<NL> &s, bool even, uint32_t scale)
{
    Big<NL> t = r;
    big_add(t, mm);
    if (twice) big_add(t, mm);
    if (scale != 1u) big_mul(t, scale);
    const int c = big_cmp(t, s);
    return even ? c >= 0 : c > 0;
}

// The digits of the finite positive double M 2^E (2^52 <= M < 2^53).  Returns their number n (1 .. 17); digit i (the first
// is i = 0) is nibble i of *lo for i < 16 and *hi for i = 16; *k: the value is 0.d0 d1 d2 ... x 10^k.
template <int NL> CPC_TEXT_HD int shortest_digits(uint64_t M, int E, uint64_t *lo, uint32_t *hi, int *k_out)
{
    const bool even = (M & 1u) == 0;
    const bool twice = M == (1ull << 52);               // a power of two: the double below is half as far as the one above
    const int extra = twice ? 2 : 1;
    Big<NL> r, s, mm;
    if (E >= 0) {
        big_set(r, M, E + extra);
        big_set(s, 1, extra);
        big_set(mm, 1, E);
    } else {
        big_set(r, M, extra);
        big_set(s, 1, extra - E);
        big_set(mm, 1, 0);
    }
    // 10^(k - 1) <= v < 10^k up to the gap: start from floor(log10(2^p)) of the leading bit p, which is floor(log10 v) or one
    // less, and let the two exact loops below settle it
    const int p = E + 52;
    int k = ((p * 78913) >> 18) + 1;                    // (78913 / 2^18 = log10(2) to 7 digits; the shift floors for p < 0 too)
    if (k > 0) big_mul_pow10(s, k);
    else if (k < 0) { big_mul_pow10(r, -k); big_mul_pow10(mm, -k); }
    while (reaches(r, mm, twice, s, even, 1u)) { big_mul(s, 10u); ++k; }
    while (!reaches(r, mm, twice, s, even, 10u)) { big_mul(r, 10u); big_mul(mm, 10u); --k; }

    const double inv_s = 1.0 / big_to_double(s);
    uint64_t dlo = 0;
    uint32_t dhi = 0;
    int n = 0;
    for (;;) {
        big_mul(r, 10u);
        big_mul(mm, 10u);
        // floor(r / s) in [0, 9]: the estimate is pushed below the quotient (its error is < 1e-12) and is then at most one short
        const double est = big_to_double(r) * inv_s - 1e-6;
        uint32_t d = est > 0.0 ? (uint32_t)est : 0u;
        if (d > 9u) d = 9u;
        big_submul(r, s, d);
        if (big_cmp(r, s) >= 0) { big_sub(r, s); ++d; }
        CPC_TEXT_CHECK(d <= 9u && big_cmp(r, s) < 0);
        const int cl = big_cmp(r, mm);
        const bool low = even ? cl <= 0 : cl < 0;
        const bool high = reaches(r, mm, twice, s, even, 1u);
        bool last = low || high;
        if (last) {
            if (high && low) {                          // both neighbours would do: the closer, an exact tie to the even digit
                Big<NL> t = r;
                big_add(t, r);
                const int c = big_cmp(t, s);
                if (c > 0 || (c == 0 && (d & 1u))) ++d;
            } else if (high) {
                ++d;
            }
            CPC_TEXT_CHECK(d <= 9u);
        }
        if (n < 16) dlo |= (uint64_t)d << (4 * n);
        else dhi = d;
        ++n;
        CPC_TEXT_CHECK(n <= 17);
        if (last || n == 17) break;
    }
    *lo = dlo;
    *hi = dhi;
    *k_out = k;
    return n;
}

// The text under construction: 24 bytes in three words, byte i of the text is byte i % 8 of word i / 8.
struct Slot {
    uint64_t w0 = 0, w1 = 0, w2 = 0;
    int len = 0;
    CPC_TEXT_HD void put(uint32_t ch)
    {
        const uint64_t v = (uint64_t)ch << (8 * (len & 7));
        const int q = len >> 3;
        if (q == 0) w0 |= v;
        else if (q == 1) w1 |= v;
        else w2 |= v;
        ++len;
    }
    CPC_TEXT_HD uint32_t byte(int i) const
    {
        const int q = i >> 3;
        const uint64_t w = q == 0 ? w0 : (q == 1 ? w1 : w2);
        return (uint32_t)(w >> (8 * (i & 7))) & 0xffu;
    }
};

// repr(float(v)) of the float with these bits
CPC_TEXT_HD Slot format_f32_bits(uint32_t bits)
{
    Slot out;
    const uint32_t mag = bits & 0x7fffffffu;
    if (mag > 0x7f800000u) { out.put('n'); out.put('a'); out.put('n'); return out; }
    if (bits >> 31) out.put('-');
    if (mag == 0x7f800000u) { out.put('i'); out.put('n'); out.put('f'); return out; }
    if (mag == 0u) { out.put('0'); out.put('.'); out.put('0'); return out; }

    const uint32_t e8 = mag >> 23, f = mag & 0x7fffffu;
    uint64_t m = e8 == 0 ? f : (f | 0x800000u);
    int E = e8 == 0 ? -149 : (int)e8 - 150;
    const int top = 31 - __builtin_clz((uint32_t)m);     // m's leading bit (m != 0, m < 2^24)
    m <<= 52 - top;                                     // the double's 53-bit significand
    E -= 52 - top;

    uint64_t lo;
    uint32_t hi;
    int k;
    const int n = (E >= -118 && E <= 58) ? shortest_digits<4>(m, E, &lo, &hi, &k) : shortest_digits<8>(m, E, &lo, &hi, &k);
    const int x = k - 1;                                // decimal exponent of the first digit
    auto digit = [&](int i) -> uint32_t { return '0' + (i < 16 ? (uint32_t)(lo >> (4 * i)) & 15u : hi); };
    if (x >= -4 && x < 16) {
        if (x < 0) {
            out.put('0'); out.put('.');
            for (int i = 0; i < -x - 1; ++i) out.put('0');
            for (int i = 0; i < n; ++i) out.put(digit(i));
        } else if (n <= x + 1) {
            for (int i = 0; i < n; ++i) out.put(digit(i));
            for (int i = n; i < x + 1; ++i) out.put('0');
            out.put('.'); out.put('0');
        } else {
            for (int i = 0; i < n; ++i) {
                if (i == x + 1) out.put('.');
                out.put(digit(i));
            }
        }
    } else {
        out.put(digit(0));
        if (n > 1) out.put('.');
        for (int i = 1; i < n; ++i) out.put(digit(i));
        out.put('e');
        out.put(x < 0 ? '-' : '+');
        const uint32_t ax = (uint32_t)(x < 0 ? -x : x);              // <= 45 for a float
        out.put('0' + ax / 10u);
        out.put('0' + ax % 10u);
    }
    return out;
}

// str(int(v))
CPC_TEXT_HD Slot format_i64(int64_t v)
{
    Slot out;
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    if (v < 0) out.put('-');
    int nd = 1;
    for (uint64_t t = u; t >= 10u; t /= 10u) ++nd;
    uint64_t div = 1;
    for (int i = 1; i < nd; ++i) div *= 10u;
    for (int i = 0; i < nd; ++i) {
        out.put('0' + (uint32_t)(u / div));
        u %= div;
        div /= 10u;
    }
    return out;
}

}  // namespace text
}  // namespace cpc
