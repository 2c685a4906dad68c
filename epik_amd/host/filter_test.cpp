// filter_test.cpp -- a stand-alone check of filter.cpp (the host mirror of the informativeness ranking), built with the
// sanitizers by `make sanitize-filter`: the math functions at their edges, hand-derived values, a forged database with
// lists around the chain count on one thread and several, the refusals.  Prints "filter selftest ok" and returns 0, or
// says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "filter.hpp"

using namespace epik_amd;

namespace {

int failures = 0;

void expect(bool ok, const char *what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

struct Csr {
    std::vector<uint32_t> keys;
    std::vector<uint64_t> offsets{0};
    std::vector<epik_amd_pkdb_value> values;
    void add(const std::vector<float> &scores)
    {
        keys.push_back((uint32_t)keys.size() * 3 + 1);
        for (size_t i = 0; i < scores.size(); ++i) values.push_back({(uint32_t)i, scores[i]});
        offsets.push_back(values.size());
    }
};

int rank(const Csr &db, uint32_t N, float log_thr, uint32_t filter, uint32_t threads, std::vector<double> &value, std::vector<uint32_t> &order,
         std::string &err)
{
    const uint64_t K = db.keys.size();
    value.assign(K, -1.0), order.assign(K, 0xffffffffu);
    return filter_rank_host(N, log_thr, db.keys.data(), db.offsets.data(), db.values.data(), K, filter, 7, threads, value.data(),
                            order.data(), err);
}

uint64_t next(uint64_t &state)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

}  // namespace

int main()
{
    const double inf = std::numeric_limits<double>::infinity();
    const float finf = std::numeric_limits<float>::infinity();
    // the math functions
    expect(ek_exp2(0.0) == 1.0 && ek_exp2(-0.0) == 1.0 && ek_exp2(-1.0) == 0.5 && ek_exp2(-1022.0) == std::ldexp(1.0, -1022), "exp2 of whole numbers");
    expect(ek_exp2(-1022.0000000001) == 0.0 && ek_exp2(-inf) == 0.0 && !std::signbit(ek_exp2(-inf)), "exp2 below -1022 is +0.0");
    expect(std::fabs(ek_exp2(-0.5) - std::sqrt(0.5)) < 1e-15 && std::fabs(ek_exp2(-1.5) - std::sqrt(0.125)) < 1e-15, "exp2 at the ties of rint");
    for (int e = -1022; e <= 1023; ++e) expect(ek_log2(std::ldexp(1.0, e)) == (double)e, "log2 of a power of two");
    expect(std::fabs(ek_log2(10.0) - kLog2Of10) < 1e-15 && std::fabs(ek_log2(kSqrtHalf) + 0.5) < 1e-15, "log2");
    expect(ek_log2(0.0) == -inf && ek_log2(inf) == inf && std::isnan(ek_log2(-1.0)), "log2 outside its domain");
    double x[3] = {-3.25, 0.0, 8.0}, e2[3], l2[3];
    filter_math_host(x, 3, e2, l2);
    expect(e2[2] == 256.0 && l2[2] == 3.0 && l2[1] == -inf, "filter_math_host");

    std::string err;
    std::vector<double> value, again;
    std::vector<uint32_t> order, order_again;
    // hand-derived values
    {
        Csr db;
        db.add(std::vector<float>(8, -2.5f));  // all 8 branches at one score: log2 8
        db.add({0.0f});                        // one entry at p = 1, seven at the threshold
        db.add(std::vector<float>(8, -2.5f));  // the first list again: a tie, ordered by key
        expect(rank(db, 8, -1.0f, EPIK_AMD_FILTER_MIF0, 1, value, order, err) == EPIK_AMD_OK, "hand cases rank");
        expect(std::fabs(value[0] - 3.0) < 1e-12 && value[0] == value[2], "all branches at one score give log2 N");
        const double t = 0.1, Z = 1.0 + 7 * t, want = std::log2(Z) - 7 * t * std::log2(t) / Z;
        expect(std::fabs(value[1] - want) < 1e-12, "one entry at s = 0");
        expect(order[0] == 1 && order[1] == 0 && order[2] == 2, "ties are ordered by key");
        Csr one;
        one.add({0.0f});
        expect(rank(one, 1, -1.0f, EPIK_AMD_FILTER_MIF0, 1, value, order, err) == EPIK_AMD_OK && value[0] == 0.0 && !std::signbit(value[0]),
               "N = 1 gives +0.0");
        Csr dead;
        dead.add({-finf, -finf});
        dead.add({-1.0f});
        expect(rank(dead, 5, -finf, EPIK_AMD_FILTER_MIF0, 1, value, order, err) == EPIK_AMD_OK && value[0] == inf && order[1] == 0,
               "Z = 0 gives +inf and is ranked last");
        expect(std::fabs(value[1]) < 1e-12, "a single entry and log_thr = -inf: no uncertainty");
    }
    // a forged database: every length around the chains, 1 thread against 5, all three filters
    {
        Csr db;
        uint64_t state = 99;
        const uint32_t N = 1303;
        for (int round = 0; round < 40; ++round)
            for (const uint32_t n : {1u, 2u, 3u, 4u, 5u, 63u, 64u, 65u, 127u, 128u, 129u, N}) {
                std::vector<float> scores(n);
                for (auto &s : scores) {
                    const uint64_t r = next(state) % 100;
                    s = r == 0 ? -finf : r == 1 ? 0.0f : r == 2 ? -4.0f : -(float)(next(state) % 4000) / 1000.0f;
                }
                db.add(scores);
            }
        for (const uint32_t filter : {EPIK_AMD_FILTER_BEST, EPIK_AMD_FILTER_MIF0, EPIK_AMD_FILTER_RANDOM}) {
            expect(rank(db, N, -4.0f, filter, 1, value, order, err) == EPIK_AMD_OK, "forged rank, one thread");
            expect(rank(db, N, -4.0f, filter, 5, again, order_again, err) == EPIK_AMD_OK, "forged rank, five threads");
            expect(std::memcmp(value.data(), again.data(), value.size() * sizeof(double)) == 0 && order == order_again, "threads change nothing");
            std::vector<bool> seen(order.size(), false);
            bool sorted = true;
            for (size_t i = 0; i < order.size(); ++i) {
                seen[order[i]] = true;
                expect(!std::isnan(value[i]), "no NaN");
                if (i && (value[order[i - 1]] > value[order[i]] || (value[order[i - 1]] == value[order[i]] && order[i - 1] > order[i]))) sorted = false;
            }
            expect(sorted, "order is sorted by (value, key)");
            for (const bool s : seen) expect(s, "order is a permutation");
        }
        // refusals
        expect(rank(db, N, -4.0f, 3, 1, value, order, err) == EPIK_AMD_ERR_INVALID && err.find("unknown filter 3") != std::string::npos, "unknown filter");
        Csr bad = db;
        bad.values[700].score = std::nanf("");
        bad.values[900].score = 0.5f;
        expect(rank(bad, N, -4.0f, EPIK_AMD_FILTER_RANDOM, 5, value, order, err) == EPIK_AMD_ERR_INVALID && err.find("values[700].score") != std::string::npos,
               "a NaN score");
        bad = db;
        bad.values[10].branch = N;
        expect(rank(bad, N, -4.0f, EPIK_AMD_FILTER_BEST, 1, value, order, err) == EPIK_AMD_ERR_INVALID && err.find("values[10].branch = 1303") != std::string::npos,
               "a branch that is not below N");
        bad = db;
        bad.offsets[6] = bad.offsets[5] - 1;
        expect(rank(bad, N, -4.0f, EPIK_AMD_FILTER_MIF0, 5, value, order, err) == EPIK_AMD_ERR_INVALID && err.find("offsets[6]") != std::string::npos,
               "offsets that are not ascending");
        Csr none;
        expect(rank(none, 3, -1.0f, EPIK_AMD_FILTER_MIF0, 2, value, order, err) == EPIK_AMD_OK, "K = 0");
    }
    if (failures) return 1;
    std::printf("filter selftest ok\n");
    return 0;
}
