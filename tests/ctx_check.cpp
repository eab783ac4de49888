// Host check of fcdiff_amd/csrc/fcd_knobs.h, the knob table of a context: every knob is set by its ABI name and lands in its
// own member, unknown names are refused, and the environment sets the defaults of exactly the fourteen knobs the header of
// the library documents -- through a fake getenv, so nothing here depends on the process environment.  The expectations
// below are written out by hand; nothing is derived from the table under test.  Prints one line per failure and
// "ok <checks>" at the end; exit status 1 after a failure.  Built and run by tests/test_ctx_header.py.
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../fcdiff_amd/csrc/fcd_knobs.h"

static int failures = 0;
static long checks = 0;

static void expect(bool ok, const char *what, const char *name = "") {
    ++checks;
    if (ok) return;
    ++failures;
    if (failures <= 20) printf("FAIL %s (%s)\n", what, name);
}

// what the ABI promises: name, member, the variable that sets its default ("" = none)
struct want_row {
    const char *name;
    int fcd_knobs::*i;
    double fcd_knobs::*d;
    const char *env;
};
static const want_row WANT[] = {
    {"r_path", &fcd_knobs::r_path, nullptr, "FCD_R_PATH"},
    {"r_ub", &fcd_knobs::r_ub, nullptr, "FCD_R_UB"},
    {"r_nopad", &fcd_knobs::r_nopad, nullptr, "FCD_R_NOPAD"},
    {"r_dsplit", &fcd_knobs::r_dsplit, nullptr, "FCD_R_DSPLIT"},
    {"r_coop", &fcd_knobs::r_coop, nullptr, "FCD_R_COOP"},
    {"qr_form", &fcd_knobs::qr_form, nullptr, "FCD_QR_FORM"},
    {"r_refill", &fcd_knobs::r_refill, nullptr, "FCD_R_REFILL"},
    {"r_tol", nullptr, &fcd_knobs::r_tol, "FCD_R_TOL"},
    {"f_tol", nullptr, &fcd_knobs::f_tol, "FCD_F_TOL"},
    {"f_form", &fcd_knobs::f_form, nullptr, "FCD_F_FORM"},
    {"f_pack", &fcd_knobs::f_pack, nullptr, "FCD_F_PACK"},
    {"corr_form", &fcd_knobs::corr_form, nullptr, "FCD_CORR_FORM"},
    {"tally_in_r", &fcd_knobs::tally_in_r, nullptr, "FCD_TALLY_IN_R"},
    {"r_keep_words", &fcd_knobs::r_keep_words, nullptr, "FCD_R_KEEP_WORDS"},
    {"f_records", &fcd_knobs::f_records, nullptr, ""},
    {"f_sure", &fcd_knobs::f_sure, nullptr, ""},
    {"f_runs", &fcd_knobs::f_runs, nullptr, ""},
    {"r_sure", &fcd_knobs::r_sure, nullptr, ""},
    {"r_sure_x", nullptr, &fcd_knobs::r_sure_x, ""},
    {"tally_in_f", &fcd_knobs::tally_in_f, nullptr, ""},
    {"partial_chunk", &fcd_knobs::partial_chunk, nullptr, ""},
    {"tangent_chunk", &fcd_knobs::tangent_chunk, nullptr, ""},
    {"r_poll_limit", &fcd_knobs::r_poll_limit, nullptr, ""},
    {"r_withhold", &fcd_knobs::r_withhold, nullptr, ""},
};
constexpr int N_WANT = (int)(sizeof(WANT) / sizeof(WANT[0]));
constexpr int N_ENV = 14;

static double get(const fcd_knobs &k, const want_row &w) { return w.d ? k.*w.d : (double)(k.*w.i); }

// k holds `value` in the member of row `at` (at < 0: nowhere) and 0 everywhere else
static void expect_only(const fcd_knobs &k, int at, double value, const char *what) {
    for (int j = 0; j < N_WANT; ++j) expect(get(k, WANT[j]) == (j == at ? value : 0.0), what, WANT[j].name);
}

// the fake environment: the variables that are set, and every name that was asked for
static std::vector<std::pair<std::string, std::string>> env_set;
static std::vector<std::string> env_asked;
static const char *fake_getenv(const char *name) {
    env_asked.push_back(name);
    for (const auto &kv : env_set)
        if (kv.first == name) return kv.second.c_str();
    return nullptr;
}
static fcd_knobs from_env(std::vector<std::pair<std::string, std::string>> set) {
    env_set = set;
    env_asked.clear();
    fcd_knobs k;
    memset(&k, 0x5A, sizeof(k));        // (whatever was there before is gone afterwards)
    fcd_knobs_from_env(k, fake_getenv);
    return k;
}
static std::string env_guess(const char *name) {       // "FCD_" + the name in capitals: how the fourteen are formed
    std::string s = "FCD_";
    for (const char *p = name; *p; ++p) s += (char)(*p >= 'a' && *p <= 'z' ? *p - 32 : *p);
    return s;
}

static void check_table() {
    expect(FCD_KNOB_N == N_WANT, "the table has 24 rows");
    const fcd_knobs dummy = {};
    for (int a = 0; a < FCD_KNOB_N; ++a) {
        const fcd_knob_row &r = fcd_knob_table[a];
        expect((r.i != nullptr) != (r.d != nullptr), "a row names one member, int or double", r.name);
        int known = 0;
        for (const want_row &w : WANT) known += !strcmp(w.name, r.name) ? 1 : 0;
        expect(known == 1, "a row's name is one of the 24 ABI names", r.name);
        const void *ma = r.d ? (const void *)&(dummy.*r.d) : (const void *)&(dummy.*r.i);
        for (int b = a + 1; b < FCD_KNOB_N; ++b) {
            const fcd_knob_row &q = fcd_knob_table[b];
            const void *mb = q.d ? (const void *)&(dummy.*q.d) : (const void *)&(dummy.*q.i);
            expect(strcmp(r.name, q.name) != 0, "two rows share a name", r.name);
            expect(ma != mb, "two rows share a member", r.name);
            expect(!r.env || !q.env || strcmp(r.env, q.env) != 0, "two rows share an environment name", r.name);
        }
    }
}

static void check_set() {
    const double values[] = {7.75, -3.9, 1.0, 2.0, 0.0, 1e30};
    for (int at = 0; at < N_WANT; ++at) {
        for (double v : values) {
            fcd_knobs k = {};
            const bool is_int = WANT[at].i != nullptr;
            if (is_int && v > 2e9) continue;         // ((int) of it is undefined: no caller passes one)
            expect(fcd_knobs_set(k, WANT[at].name, v), "a knob is set by its ABI name", WANT[at].name);
            expect_only(k, at, is_int ? (double)(int)v : v, "set: the value in its own member, ints truncated, and nowhere else");
        }
    }
    // r_coop = 2, the refusal test hook, is accepted here (not from the environment: below)
    fcd_knobs k = {};
    expect(fcd_knobs_set(k, "r_coop", 2.0) && k.r_coop == 2, "set: r_coop = 2 is kept");
    const char *unknown[] = {"", "nope", "r_pat", "r_path ", " r_path", "R_PATH", "FCD_R_PATH", "r_path\n", "n_alloc"};
    for (const char *name : unknown) {
        fcd_knobs z = {};
        expect(!fcd_knobs_set(z, name, 5.0), "an unknown name is refused", name);
        expect_only(z, -1, 0.0, "a refused name changes nothing");
    }
}

static void check_env() {
    // nothing set: every default 0, and exactly the fourteen variables are asked for
    expect_only(from_env({}), -1, 0.0, "empty environment: every knob at its default");
    expect((int)env_asked.size() == N_ENV, "fourteen variables are looked up");
    for (int j = 0; j < N_WANT; ++j) {
        int n = 0;
        for (const std::string &a : env_asked) n += a == env_guess(WANT[j].name) ? 1 : 0;
        expect(n == (j < N_ENV ? 1 : 0), "looked up once if it is one of the fourteen, else never", WANT[j].name);
    }
    for (int at = 0; at < N_WANT; ++at) {
        const want_row &w = WANT[at];
        const std::string var = env_guess(w.name);
        const bool has = w.env[0] != 0;
        expect(has == (at < N_ENV) && (!has || var == w.env), "the fourteen names", w.name);
        // "1": the one member where the variable is one of the fourteen, nothing otherwise
        expect_only(from_env({{var, "1"}}), has ? at : -1, 1.0, "VAR=1 sets its own knob's default and no other");
        // a fraction: ints truncated, doubles kept -- and r_coop takes 1 only
        const double want25 = !strcmp(w.name, "r_coop") ? 0.0 : (w.d ? 2.5 : 2.0);
        expect_only(from_env({{var, "2.5"}}), has ? at : -1, want25, "VAR=2.5: truncated in an int, kept in a double");
        // "0", "" and text that is no number mean the default
        expect_only(from_env({{var, "0"}}), -1, 0.0, "VAR=0 is the default");
        expect_only(from_env({{var, ""}}), -1, 0.0, "VAR= (empty) is the default");
        expect_only(from_env({{var, "x"}}), -1, 0.0, "VAR=x is the default");
    }
    expect(from_env({{"FCD_R_COOP", "2"}}).r_coop == 0, "FCD_R_COOP=2 gives 0");
    expect(from_env({{"FCD_R_COOP", "1"}}).r_coop == 1, "FCD_R_COOP=1 gives 1");
    expect(from_env({{"FCD_R_COOP", "3"}}).r_coop == 0, "FCD_R_COOP=3 gives 0");
    expect(from_env({{"FCD_R_COOP", "-1"}}).r_coop == 0, "FCD_R_COOP=-1 gives 0");
    // all fourteen at once, each with its own number
    std::vector<std::pair<std::string, std::string>> all;
    for (int j = 0; j < N_ENV; ++j) all.push_back({WANT[j].env, std::to_string(j + 1)});
    const fcd_knobs k = from_env(all);
    for (int j = 0; j < N_WANT; ++j) {
        const double want = j >= N_ENV ? 0.0 : !strcmp(WANT[j].name, "r_coop") ? 0.0 : (double)(j + 1);
        expect(get(k, WANT[j]) == want, "all fourteen set: each in its own member", WANT[j].name);
    }
}

int main() {
    check_table();
    check_set();
    check_env();
    if (failures) {
        printf("%d failures in %ld checks\n", failures, checks);
        return 1;
    }
    printf("ok %ld\n", checks);
    return 0;
}
