// Host check of the plain-C++ part of fcdiff_amd/csrc/fcd_tally.h: the bit-sliced counters of the count tallies against
// per-chain integer counts, and the CSR checks of the region sets and patient groups with their message texts.  Prints one
// line per failure and "ok <checks>" at the end; exit status 1 after a failure.  Built and run by tests/test_tally_header.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../fcdiff_amd/csrc/fcd_tally.h"

static int failures = 0;
static long checks = 0;

static void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
    ++checks;
    if (ok) return;
    ++failures;
    if (failures <= 20) printf("FAIL %s (%lld, %lld)\n", what, a, b);
}

// the counters after some adds against the 64 counts they should hold: any() and the layout "chain c at row[c]"
static void compare(const tally_planes<10> &pl, const int *want, long long step) {
    alignas(8) uint16_t row[64];
    memset(row, 0xA5, sizeof(row));
    pl.store16(row);
    const uint64_t any = pl.any();
    for (int c = 0; c < 64; ++c) {
        expect(row[c] == want[c], "store16: count of a chain", step, c);
        expect(((any >> c) & 1ull) == (want[c] > 0 ? 1ull : 0ull), "any: bit of a chain", step, c);
    }
}

static uint64_t rand64() { return ((uint64_t)mrand48() << 32) ^ (uint64_t)(uint32_t)mrand48(); }

static void check_planes() {
    tally_planes<10> pl;
    int want[64];
    // all-zero input
    pl.clear();
    memset(want, 0, sizeof(want));
    compare(pl, want, -1);
    for (int i = 0; i < 100; ++i) pl.add(0ull);
    compare(pl, want, -2);
    // every chain at once up to the largest count: 1, 511, 512 (the carry into the top plane), 1022, 1023 on the way
    for (int k = 1; k <= 1023; ++k) {
        pl.add(~0ull);
        for (int c = 0; c < 64; ++c) want[c] = k;
        if (k == 1 || k == 511 || k == 512 || k == 1022 || k == 1023 || k % 97 == 0) compare(pl, want, k);
    }
    // 64 independent chains: four runs of 1023 random words (no count can pass 1023) of bit density 1/2, 1/4, 3/4 and mixed
    srand48(7);
    for (int run = 0; run < 4; ++run) {
        pl.clear();
        memset(want, 0, sizeof(want));
        for (int i = 0; i < 1023; ++i) {
            const uint64_t a = rand64(), b = rand64();
            const int kind = run < 3 ? run : i % 3;
            const uint64_t word = kind == 0 ? a : (kind == 1 ? a & b : a | b);
            pl.add(word);
            for (int c = 0; c < 64; ++c) want[c] += (int)((word >> c) & 1ull);
            if (i % 8 == 7 || i == 1022) compare(pl, want, (long long)run * 10000 + i);
        }
    }
    // clear() after use
    pl.clear();
    memset(want, 0, sizeof(want));
    compare(pl, want, -3);
}

static char msg[256];
static int code_seen;
static int fail_as(int code, const char *fmt, long long a, long long b) {       // "<who>: <text>", as fcd_fail_who writes it
    char tail[192];
    snprintf(tail, sizeof(tail), fmt, a, b);
    snprintf(msg, sizeof(msg), "%s: %s", "who", tail);
    code_seen = code;
    return code;
}

static void refusal(const char *noun, const int32_t *offsets, const int32_t *members, int64_t J, const char *text) {
    int64_t smax = 123, max_member = 123;
    msg[0] = 0;
    code_seen = 0;
    const int rc = tally_csr_check(fail_as, noun, offsets, members, J, &smax, &max_member);
    expect(rc == FCD_ERR_ARG && code_seen == FCD_ERR_ARG, "csr: a refusal's code", rc);
    const bool same = strcmp(msg, text) == 0;
    expect(same, "csr: a refusal's text");
    if (!same) printf("  got  \"%s\"\n  want \"%s\"\n", msg, text);
}

static void check_csr() {
    {   // {0, 5}, {2}, {1, 2, 9}: accepted, and the two maxima
        const int32_t offsets[] = {0, 2, 3, 6}, members[] = {0, 5, 2, 1, 2, 9};
        int64_t smax = -7, max_member = -7;
        msg[0] = 0;
        expect(tally_csr_check(fail_as, "set", offsets, members, 3, &smax, &max_member) == FCD_OK, "csr: accepted");
        expect(smax == 3 && max_member == 9, "csr: largest size and member", smax, max_member);
        expect(msg[0] == 0, "csr: no message when accepted");
    }
    const int32_t m01[] = {0, 1}, neg[] = {-1, 3}, dup[] = {3, 3}, down[] = {1, 3, 2}, late[] = {0, 1, 4, 4};
    const int32_t o_first[] = {1, 2}, o_empty[] = {0, 1, 1}, o_back[] = {0, 2, 1}, o2[] = {0, 2}, o3[] = {0, 3}, o22[] = {0, 2, 4};
    refusal("set", o_first, m01, 1, "who: offsets[0]=1");
    refusal("set", o_empty, m01, 2, "who: set 1 is empty");
    refusal("set", o_back, m01, 2, "who: set 1 is empty");
    refusal("set", o2, neg, 1, "who: set 0 has the negative member -1");
    refusal("set", o2, dup, 1, "who: the members of set 0 do not increase at 3");
    refusal("set", o3, down, 1, "who: the members of set 0 do not increase at 2");
    refusal("set", o22, late, 2, "who: the members of set 1 do not increase at 4");
    refusal("group", o_empty, m01, 2, "who: group 1 is empty");
    refusal("group", o2, neg, 1, "who: group 0 has the negative member -1");
    refusal("group", o3, down, 1, "who: the members of group 0 do not increase at 2");
}

int main() {
    check_planes();
    check_csr();
    if (!failures) printf("ok %ld\n", checks);
    return failures ? 1 : 0;
}
