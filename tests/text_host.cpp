// Host build of cpc2_amd/csrc/text_digits.h for tests/test_export_cpu.py: the arithmetic the kernels of text.hip run, compiled
// for the CPU with every "this carry is zero" condition turned into a counted failure.
#include <cstdint>
#include <cstring>
static long g_failed = 0;
#define CPC_TEXT_CHECK(cond) do { if (!(cond)) ++g_failed; } while (0)
#include "../cpc2_amd/csrc/text_digits.h"

static void store(const cpc::text::Slot &s, unsigned char *slots, unsigned char *len, long i)
{
    const uint64_t w[3] = {s.w0, s.w1, s.w2};
    std::memcpy(slots + cpc::text::SLOT_BYTES * i, w, cpc::text::SLOT_BYTES);
    len[i] = (unsigned char)s.len;
}
extern "C" long text_host_f32(const uint32_t *bits, long count, unsigned char *slots, unsigned char *len)
{
    g_failed = 0;
    for (long i = 0; i < count; ++i) store(cpc::text::format_f32_bits(bits[i]), slots, len, i);
    return g_failed;
}
// the 8-word path alone, for every pattern (the kernels take it only where 4 words do not suffice)
extern "C" long text_host_digits8(const uint32_t *bits, long count, unsigned long long *lo, unsigned *hi, int *n, int *k)
{
    g_failed = 0;
    for (long i = 0; i < count; ++i) {
        const uint32_t mag = bits[i] & 0x7fffffffu, e8 = mag >> 23, f = mag & 0x7fffffu;
        if (mag == 0 || mag >= 0x7f800000u) { n[i] = 0; continue; }
        uint64_t m = e8 == 0 ? f : (f | 0x800000u);
        int E = e8 == 0 ? -149 : (int)e8 - 150;
        const int top = 31 - __builtin_clz((uint32_t)m);
        m <<= 52 - top;
        E -= 52 - top;
        uint64_t l; uint32_t h; int kk;
        n[i] = cpc::text::shortest_digits<8>(m, E, &l, &h, &kk);
        lo[i] = l; hi[i] = h; k[i] = kk;
    }
    return g_failed;
}
extern "C" long text_host_i64(const int64_t *v, long count, unsigned char *slots, unsigned char *len)
{
    g_failed = 0;
    for (long i = 0; i < count; ++i) store(cpc::text::format_i64(v[i]), slots, len, i);
    return g_failed;
}
