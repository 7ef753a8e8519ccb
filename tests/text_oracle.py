"""The integer statement of what cpc2_amd/csrc/text_digits.h computes, in Python's unbounded integers: Steele & White's
free-format digit generation for the DOUBLE equal to a float32, and repr's layout of the digits.  tests/test_export_cpu.py
holds it against CPython's own repr; the GPU tests hold the kernels against repr directly."""
import struct

import numpy as np

TIES = (0xc2ce6f44, 0xc4647159, 0x443baac5)          # exact ties between two shortest strings: the even digit wins


def bits_of(value):
    return struct.unpack("<I", struct.pack("<f", value))[0]


def digits_f32(bits):
    """(digits, k) of the finite positive float32 with these bits: the value is 0.d1 d2 ... x 10^k."""
    e8, f = (bits >> 23) & 0xff, bits & 0x7fffff
    m, e = (f, -149) if e8 == 0 else (f | 0x800000, e8 - 150)
    shift = 53 - m.bit_length()                      # as a double: 53-bit significand M, exponent E
    M, E = m << shift, e - shift
    even = M & 1 == 0
    twice = M == 1 << 52                             # a power of two: the gap below is half the gap above
    extra = 2 if twice else 1
    # r / s = the value, mp / s and mm / s = half the gap to the next double above / below
    if E >= 0:
        r, s, mp, mm = M << (E + extra), 1 << extra, (2 if twice else 1) << E, 1 << E
    else:
        r, s, mp, mm = M << extra, 1 << (extra - E), 2 if twice else 1, 1

    def reaches(r, mp, s):
        return r + mp >= s if even else r + mp > s

    k = 0
    while reaches(r, mp, s):
        s *= 10
        k += 1
    while not reaches(10 * r, 10 * mp, s):
        r, mp, mm = 10 * r, 10 * mp, 10 * mm
        k -= 1
    out = []
    while True:
        r, mp, mm = 10 * r, 10 * mp, 10 * mm
        d, r = divmod(r, s)
        low = r <= mm if even else r < mm
        high = reaches(r, mp, s)
        if low or high:
            break
        out.append(d)
    if low and high:                                 # the closer of the two; an exact tie goes to the even digit
        d += 1 if 2 * r > s or (2 * r == s and d % 2 == 1) else 0
    elif high:
        d += 1
    out.append(d)
    return out, k


def layout(sign, digits, k):
    """repr's layout of the digits 0.d1 d2 ... x 10^k."""
    s = "".join(map(str, digits))
    n, x = len(s), k - 1                             # x: the decimal exponent of the first digit
    if -4 <= x < 16:
        if x < 0:
            body = "0." + "0" * (-x - 1) + s
        elif n <= x + 1:
            body = s + "0" * (x + 1 - n) + ".0"
        else:
            body = s[:x + 1] + "." + s[x + 1:]
    else:
        body = s[0] + ("." + s[1:] if n > 1 else "") + "e" + ("-" if x < 0 else "+") + "%02d" % abs(x)
    return sign + body


def format_bits(bits):
    """The text of the float32 with these bits."""
    sign, mag = "-" if bits >> 31 else "", bits & 0x7fffffff
    if mag > 0x7f800000:
        return "nan"
    if mag == 0x7f800000:
        return sign + "inf"
    if mag == 0:
        return sign + "0.0"
    return layout(sign, *digits_f32(mag))


def fixed_patterns():
    """The issue's fixed list as uint32 bit patterns."""
    named = [0x00000000, 0x80000000,                  # +-0
             0x00000001, 0x007fffff,                  # the smallest and the largest subnormal
             0x00800000, 0x7f7fffff,                  # the smallest normal, the largest finite value
             0x7f800000, 0xff800000, 0x7fc00000,      # +-inf, nan
             0x80000001, 0x80800000, 0xff7fffff, 0xffc00000, 0x7f800001]
    values = [1.0, 1e-5, 9.9999e-5, 1e-4, 9.99e15, 1e16, 1e22, 16777216.0]
    named += [bits_of(v) for v in values] + [bits_of(-v) for v in values]
    powers = [e << 23 for e in range(1, 255)] + [1 << b for b in range(23)]          # every power of two, 2^-149 .. 2^127
    return np.array(named + powers + list(TIES), dtype=np.uint32)


def random_patterns(count, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, count, dtype=np.uint64).astype(np.uint32)


def repr_of(bits):
    """CPython's text of every pattern: the contract."""
    return [repr(float(v)) for v in np.asarray(bits, dtype=np.uint32).view(np.float32)]


def rows_text(matrix_texts, prefix=None):
    """The bytes format_rows must give for a matrix of value texts (a list of rows of strings)."""
    lines = []
    for r, row in enumerate(matrix_texts):
        head = [] if prefix is None else [prefix[r].decode() if isinstance(prefix[r], bytes) else prefix[r]]
        lines.append(" ".join(head + list(row)) + "\n")
    return "".join(lines).encode()
