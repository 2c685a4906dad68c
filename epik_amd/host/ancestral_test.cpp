// ancestral_test.cpp -- a stand-alone check of ancestral.cpp (the host mirror of the ancestral reconstruction and the
// model side), built with the sanitizers by `make sanitize-ancestral`: a tree of four leaves and a caterpillar of sixty
// under GTR with gamma categories and invariant sites, gaps and ambiguity codes at the leaves; the checks' refusals.
// Prints "ancestral selftest ok" and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ancestral.hpp"

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

struct Case {
    std::vector<int32_t> parent;
    std::vector<double> length, weights, pi, full, half, pend;
    std::vector<uint32_t> masks;
    uint32_t C = 0;
    uint64_t L = 0;
    epik_amd_ancestral_desc desc{};
};

// tables of a tree under GTR + G4 + I; the pendant length is taken as the branch's own (any length serves here)
void fill(Case &c, uint64_t L)
{
    const uint32_t N = (uint32_t)c.parent.size(), S = 4;
    const double exchange[6] = {1.3, 4.1, 0.7, 1.1, 5.2, 1.0};
    c.pi = {0.31, 0.19, 0.22, 0.28};
    double rates[4];
    std::string err;
    expect(model_gamma_rates(0.6, 4, rates, err) == EPIK_AMD_OK, "gamma rates");
    const double p_inv = 0.15;
    c.C = 5, c.L = L;
    c.weights.assign(5, (1.0 - p_inv) / 4);
    c.weights[4] = p_inv;
    std::vector<double> cat(5, 0.0);
    for (int i = 0; i < 4; ++i) cat[i] = rates[i] / (1.0 - p_inv);
    std::vector<double> times((size_t)(N - 1) * c.C), halves(times.size());
    for (uint32_t b = 0; b + 1 < N; ++b)
        for (uint32_t k = 0; k < c.C; ++k) times[(size_t)b * c.C + k] = c.length[b] * cat[k], halves[(size_t)b * c.C + k] = c.length[b] / 2 * cat[k];
    c.full.resize(times.size() * S * S), c.half.resize(c.full.size()), c.pend.resize(c.full.size());
    expect(model_pmatrices(S, exchange, c.pi.data(), times.data(), times.size(), c.full.data(), err) == EPIK_AMD_OK, "p_full");
    expect(model_pmatrices(S, exchange, c.pi.data(), halves.data(), halves.size(), c.half.data(), err) == EPIK_AMD_OK, "p_half");
    c.pend = c.full;
    uint32_t leaves = 0;
    std::vector<bool> inner(N, false);
    for (uint32_t v = 0; v + 1 < N; ++v) inner[c.parent[v]] = true;
    for (uint32_t v = 0; v < N; ++v) leaves += !inner[v];
    c.masks.resize((size_t)leaves * L);
    uint32_t x = 12345;
    for (auto &m : c.masks) {
        x = x * 1664525u + 1013904223u;
        const uint32_t r = x >> 24;
        m = r < 16 ? 0u : r < 32 ? 5u : r < 40 ? 15u : 1u << (r & 3);
    }
    c.desc = epik_amd_ancestral_desc{N, S, c.C, 0, c.parent.data(), c.weights.data(), c.pi.data(), c.full.data(), c.half.data(), c.pend.data()};
}

void run(Case &c, const char *name)
{
    std::string err;
    ancestral_tree tree;
    expect(ancestral_check(c.desc, tree, err) == EPIK_AMD_OK, name);
    if (failures) {
        std::printf("%s: %s\n", name, err.c_str());
        return;
    }
    const uint32_t N = c.desc.num_nodes;
    const uint64_t G = ancestral_ghost_count(N, EPIK_AMD_GHOSTS_BOTH);
    std::vector<float> one(G * c.L * 4, -1.0f), many(one.size(), -2.0f);
    uint64_t dead_one = 99, dead_many = 99;
    ancestral_rule_host(c.desc, tree, c.masks.data(), c.L, EPIK_AMD_GHOSTS_BOTH, 1, one.data(), &dead_one);
    ancestral_rule_host(c.desc, tree, c.masks.data(), c.L, EPIK_AMD_GHOSTS_BOTH, 5, many.data(), &dead_many);
    expect(dead_one == 0 && dead_many == 0, "no dead row");
    expect(std::memcmp(one.data(), many.data(), one.size() * sizeof(float)) == 0, "threads cannot change a bit");
    for (uint64_t r = 0; r < G * c.L; ++r) {
        float sum = 0;
        for (int s = 0; s < 4; ++s) sum += one[r * 4 + s];
        if (!(std::fabs(sum - 1.0f) <= 1e-6f)) {
            expect(false, "a row sums to 1");
            break;
        }
    }
    // the halves alone
    std::vector<float> inner((G / 2) * c.L * 4), outer(inner.size());
    ancestral_rule_host(c.desc, tree, c.masks.data(), c.L, EPIK_AMD_GHOSTS_INNER, 2, inner.data(), nullptr);
    ancestral_rule_host(c.desc, tree, c.masks.data(), c.L, EPIK_AMD_GHOSTS_OUTER, 2, outer.data(), nullptr);
    expect(std::memcmp(inner.data(), one.data(), inner.size() * sizeof(float)) == 0, "inner is the first half of both");
    expect(std::memcmp(outer.data(), one.data() + inner.size(), outer.size() * sizeof(float)) == 0, "outer is the second half of both");
    std::vector<uint32_t> branch_of(G);
    ancestral_branch_of(N, EPIK_AMD_GHOSTS_BOTH, branch_of.data());
    expect(branch_of[0] == 0 && branch_of[G / 2] == 0 && branch_of[G - 1] == N - 2, "branch_of");
}

}  // namespace

int main()
{
    Case four;
    four.parent = {2, 2, 6, 5, 5, 6, -1};
    four.length = {0.11, 0.23, 0.07, 0.4, 0.0, 0.19};
    fill(four, 37);
    run(four, "four leaves");

    Case cat;  // (((l0, l1), l2), ...): leaves 0, 1, 3, 5, ...; inner nodes 2, 4, 6, ...
    const uint32_t leaves = 60, N = 2 * leaves - 1;
    cat.parent.assign(N, -1);
    cat.parent[0] = 2, cat.parent[1] = 2;
    for (uint32_t v = 2; v + 1 < N; ++v) cat.parent[v] = v % 2 == 0 ? v + 2 : v + 1;
    cat.length.assign(N - 1, 5.0);
    fill(cat, 9);
    run(cat, "caterpillar");

    // refusals
    std::string err;
    ancestral_tree tree;
    Case bad = four;
    bad.desc.parent = bad.parent.data();
    bad.parent[2] = 1;
    expect(ancestral_check(bad.desc, tree, err) == EPIK_AMD_ERR_INVALID && err.find("not a later node") != std::string::npos, "post-order is checked");
    bad = four;
    bad.half[5] = std::nan("");
    bad.desc.p_half = bad.half.data();
    expect(ancestral_check(bad.desc, tree, err) == EPIK_AMD_ERR_INVALID && err.find("p_half[0][0][1][1]") != std::string::npos, "tables are checked");
    expect(ancestral_check_call(nullptr, 3, 0, err) == EPIK_AMD_ERR_INVALID, "null masks");
    expect(ancestral_check_call(four.masks.data(), 3, 7, err) == EPIK_AMD_ERR_INVALID, "ghost choice");
    double out[16];
    const double pi0[4] = {0.5, 0.5, 0.0, 0.0}, ex[6] = {1, 1, 1, 1, 1, 1}, t = 0.1;
    expect(model_pmatrices(4, ex, pi0, &t, 1, out, err) == EPIK_AMD_ERR_INVALID, "a frequency of 0 is refused");
    expect(model_gamma_rates(-1.0, 4, out, err) == EPIK_AMD_ERR_INVALID && model_gamma_rates(1.0, 9, out, err) == EPIK_AMD_ERR_INVALID, "gamma arguments");
    for (const double alpha : {0.02, 0.5, 1.0, 7.0, 200.0})
        for (uint32_t K = 1; K <= 8; ++K) {
            double rates[8], sum = 0;
            expect(model_gamma_rates(alpha, K, rates, err) == EPIK_AMD_OK, "gamma rates");
            for (uint32_t i = 0; i < K; ++i) sum += rates[i];
            expect(std::fabs(sum / K - 1.0) < 1e-12, "gamma mean");
        }
    expect(std::fabs(gamma_p(1.0, 2.0) - (1.0 - std::exp(-2.0))) < 1e-14 && gamma_p(2.0, 0.0) == 0.0, "gamma_p");
    expect(std::fabs(gamma_p_inverse(1.0, 0.5) - std::log(2.0)) < 1e-14, "gamma_p_inverse");
    if (failures) return 1;
    std::printf("ancestral selftest ok\n");
    return 0;
}
