// Stand-alone host program (tests/test_dataset_mask_cpu.py builds it with -fsanitize=address,undefined): the group functions of
// csrc/hk_maskbits_core.h -- what every lane of dataset_mask_kernel runs -- over rows of width 1 .. 130, both kinds of validity
// (packed bits, an alpha row), every sample type, against a loop over the pixels that knows nothing of groups.  Every row lives in
// a heap block of exactly its size, so a load or a store of a group outside [row, row + width), or outside ceil(width / 8) bytes
// of a mask row, is the sanitizer's finding; the host build of the wide accesses aborts on an address the header did not promise.
// Rows are tried at an address that allows the wide path and at one that does not (one sample further).
// Prints one line per kind and returns 0, or the failed checks and 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#define HKM_HOST
#include "hk_maskbits_core.h"

using namespace hk::maskbits;

static int failures = 0;
static long long rows_checked[2] = {0, 0}, wide_groups = 0, narrow_groups = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

template <typename T>
static T sample(int i) {
    if (sizeof(T) == 8) {   // float64: values float32 holds, values it rounds, values past its range, a NaN
        const double v[] = {0.0, -0.0, 1.5, 16777217.0, 1e39, -1e39, 1e-46, (double)NAN, 0.1};
        return (T)v[(rnd() + i) % 9];
    }
    T t;
    const uint32_t r = rnd();
    memcpy(&t, &r, sizeof t);   // any bit pattern: a float32 NaN of any payload included
    return t;
}

// a row of n elements in a heap block of exactly n (+ shift) elements, `shift` elements into it
template <typename T>
struct Row {
    T* block;
    T* p;
    Row(long long n, int shift) : block((T*)malloc((size_t)(n + shift) * sizeof(T))), p(block + shift) {}
    ~Row() { free(block); }
};

template <typename T, int KIND>
static void one_row(int width, int shift, int pattern) {
    using A = typename std::conditional<KIND == KIND_ALPHA, T, unsigned char>::type;
    const long long groups = groups_of(width), vlen = KIND == KIND_BITS ? groups : width;
    Row<T> in(width, shift);
    Row<A> v(vlen, KIND == KIND_ALPHA ? shift : 0);
    Row<float> out(width, shift ? 1 : 0), want(width, 0);
    for (int x = 0; x < width; ++x) in.p[x] = sample<T>(x);
    for (long long k = 0; k < vlen; ++k) {
        const uint32_t r = rnd();
        v.p[k] = (A)(pattern == 0 ? ~0u : pattern == 1 ? 0u : (KIND == KIND_ALPHA ? ((r & 1) ? r >> 8 : 0u) : r));
    }
    const uint32_t canary = 0xA5A5A5A5u;
    for (int x = 0; x < width; ++x) memcpy(out.p + x, &canary, 4);
    // the statement: pixel by pixel
    for (int x = 0; x < width; ++x) {
        const bool valid = KIND == KIND_BITS ? ((v.p[x / 8] >> (7 - x % 8)) & 1) != 0 : v.p[x] != 0;
        const float f = valid ? (float)in.p[x] : 0.f;
        uint32_t b = NAN_BITS;
        if (valid) memcpy(&b, &f, 4);
        memcpy(want.p + x, &b, 4);
    }
    // the header: group by group, as the kernel calls it
    for (long long g = 0; g < groups; ++g) {
        const bool whole = g * GROUP + GROUP <= width;
        unsigned valid;
        if (KIND == KIND_BITS) valid = bits_group((const unsigned char*)v.p, g);
        else valid = alpha_group<A>(v.p, g, width, whole && row_wide<A>(v.p));
        const bool wide = whole && row_wide<T>(in.p) && out_row_wide(out.p);
        (wide ? wide_groups : narrow_groups) += 1;
        put_group<T>(in.p, out.p, g, width, valid, wide);
    }
    if (memcmp(out.p, want.p, (size_t)width * 4) != 0) {
        ++failures;
        fprintf(stderr, "FAILED kind %d, %zu-byte samples, width %d, shift %d, pattern %d\n", KIND, sizeof(T), width, shift, pattern);
    }
    ++rows_checked[KIND];
}

template <typename T, int KIND>
static void sweep() {
    for (int width = 1; width <= 130; ++width)
        for (int shift = 0; shift < 2; ++shift)
            for (int pattern = 0; pattern < 3; ++pattern) one_row<T, KIND>(width, shift, pattern);
}

int main() {
    sweep<float, KIND_BITS>(), sweep<unsigned char, KIND_BITS>(), sweep<unsigned short, KIND_BITS>(), sweep<short, KIND_BITS>();
    sweep<unsigned int, KIND_BITS>(), sweep<int, KIND_BITS>(), sweep<double, KIND_BITS>();
    sweep<unsigned char, KIND_ALPHA>(), sweep<unsigned short, KIND_ALPHA>();
    printf("bits: %lld rows\nalpha: %lld rows\n", rows_checked[0], rows_checked[1]);
    if (wide_groups == 0 || narrow_groups == 0) {
        ++failures;
        fprintf(stderr, "FAILED: %lld wide and %lld narrow groups: both paths must have run\n", wide_groups, narrow_groups);
    }
    return failures ? 1 : 0;
}
