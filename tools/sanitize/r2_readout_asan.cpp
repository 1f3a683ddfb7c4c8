// Stand-alone sanitizer driver (host code only, never on a GPU): the emulated register-resident 2-state body (tests/emul/emul_gform.cpp and, for
// the GAPS instantiation, tests/emul/emul_r2_gap.cpp -> csrc/xt_reg2.h: xt_r2_body) over the shapes of tests/r2_readout_cases.py: the lengths
// around the window and the staging chunks for F 4, 6, 7 x D 1, 2, 3; at D = 2 also outliers in the last row and from row L - 2 on, a NaN
// coordinate, N = 1 and N = tracks-per-wave + 1; the small-l2 triples; 25 % missed rows with a missed row at L - 2 (GAPS).  Every launch with and
// without per-track output.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sanitize/r2_readout_asan.cpp -o /tmp/r2_readout_asan && /tmp/r2_readout_asan
#include "../../tests/emul/emul_gform.cpp"
#include "../../tests/emul/emul_r2_gap.cpp"
#include <cstdio>
#include <random>

static std::vector<double> walk(std::mt19937_64& g, long long N, int L, int D)
{
    std::normal_distribution<double> nd(0.0, 0.08);
    std::vector<double> c((size_t)N * L * D);
    for (long long n = 0; n < N; ++n)
        for (int d = 0; d < D; ++d) {
            double x = 0.0;
            for (int t = 0; t < L; ++t) c[((size_t)n * L + t) * D + d] = (x += nd(g));
        }
    return c;
}

static const double ds[2] = {0.004, 0.1}, Fs[2] = {.35, .65}, T[4] = {.92, .08, .15, .85}, ps[2] = {0.99, 0.9};
static int launches = 0, bad = 0;

// one g-form launch, with and without per-track output; want_nan: a poisoned track makes the total NaN
static void gform(const char* what, std::vector<double>& c, long long n, int L, int D, int F, double le, bool want_nan)
{
    const double lev[3] = {le, 0, 0};
    for (int per_track = 0; per_track < 2; ++per_track) {
        std::vector<double> ll(n, 0.0);
        double tot = 0.0;
        int scaling = -1;
        const int rc = xt_emul_gform_run(c.data(), nullptr, n, L, D, 1, F, 1, 3, 0, 1, lev, 0.1, ds, Fs, T, ps, n > 1 ? 2 : 1, 0, per_track ? ll.data() : nullptr, &tot, &scaling);
        ++launches;
        if (rc != 0 || scaling != 2 || (std::isnan(tot) != want_nan) || (!want_nan && !std::isfinite(tot))) {
            ++bad;
            printf("%s F=%d D=%d L=%d N=%lld per_track=%d: rc %d scaling %d total %g\n", what, F, D, L, n, per_track, rc, scaling, tot);
        }
    }
}

int main()
{
    std::mt19937_64 g(1);
    for (int F : {4, 6, 7})
        for (int D : {1, 2, 3}) {
            const int tpw = 64 >> (F - 1);
            const long long N = 2 * tpw * 4 + 1;
            std::vector<int> Ls = {3, F, F + 1, 32, 33, 34, 65};
            for (int L = F + 2; L <= 2 * F; ++L) Ls.push_back(L);
            for (int L : Ls) {
                std::vector<double> c = walk(g, N, L, D);
                gform("lengths", c, N, L, D, F, 0.02, false);
                if (D != 2) continue;
                for (int from : {L - 1, L - 2}) {  // outliers: + 20, one track + 520
                    c = walk(g, N, L, D);
                    for (long long i = 0; i < N; ++i)
                        for (int t = from; t < L; ++t)
                            for (int d = 0; d < D; ++d) c[((size_t)i * L + t) * D + d] += i == 3 ? 520.0 : 20.0;
                    gform(from == L - 1 ? "last-row outlier" : "outlier from L-2", c, N, L, D, F, 0.02, false);
                }
                c = walk(g, N, L, D);
                c[((size_t)1 * L + L - 1) * D] = NAN;
                gform("NaN", c, N, L, D, F, 0.02, true);
                for (long long n : {1LL, (long long)tpw + 1}) {
                    c = walk(g, n, L, D);
                    gform("single tracks", c, n, L, D, F, 0.02, false);
                }
            }
        }
    const struct { int F, D; double le; } small[3] = {{6, 3, 1e-5}, {7, 3, 2e-6}, {4, 2, 1e-5}};
    for (const auto& sc : small)
        for (int L : {sc.F + 2, 33}) {
            std::vector<double> c = walk(g, 2 * (64 >> (sc.F - 1)) * 4 + 1, L, sc.D);
            gform("small l2", c, 2 * (64 >> (sc.F - 1)) * 4 + 1, L, sc.D, sc.F, sc.le, false);
        }
    // GAPS: 25 % of the interior rows missed, row L - 2 missed on tracks 1 and 2
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int F : {4, 6, 7})
        for (int D : {1, 2, 3})
            for (int L : {F + 2, 12, 33}) {
                const long long N = std::max(2 * (64 >> (F - 1)) * 4 + 1, 9);
                std::vector<double> c = walk(g, N, L, D);
                for (long long i = 0; i < N; ++i)
                    for (int t = 1; t < L - 1; ++t)
                        if ((i > 1 && u(g) < 0.25) || ((i == 1 || i == 2) && t == L - 2))
                            for (int d = 0; d < D; ++d) c[((size_t)i * L + t) * D + d] = NAN;
                for (int per_track = 0; per_track < 2; ++per_track) {
                    std::vector<double> ll(N, 0.0);
                    double tot = 0.0;
                    int info[4] = {0, 0, 0, 0};
                    const int rc = xt_emul_r2_gap_run(c.data(), N, L, D, F, 1, 3, 0.02, 0.1, ds, Fs, T, ps, 2, 1, 1, 0xf0, per_track ? ll.data() : nullptr, &tot, info);
                    ++launches;
                    if (rc != 0 || info[0] != XT_LL_GAPS_REG2 || !std::isfinite(tot)) {
                        ++bad;
                        printf("gaps F=%d D=%d L=%d per_track=%d: rc %d path %d total %g\n", F, D, L, per_track, rc, info[0], tot);
                    }
                }
            }
    printf("%d launches, %d bad\n", launches, bad);
    return bad != 0;
}
