// build.cpp -- the host mirror of the database builder (build.hpp): pruned depth-first enumeration of every window
// of every ghost node, then a std::sort of the (key, branch, score) tuples and one pass that keeps the best of each run.
#include "build.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>
#include <utility>

namespace epik_amd {

namespace {

int invalid(std::string &err, const std::string &what)
{
    err = what;
    return EPIK_AMD_ERR_INVALID;
}

struct Tuple {
    uint64_t packed;
    float score;
};

// one window: the letters of position d .. k - 1 below a prefix of sum s
struct Walker {
    uint32_t sigma, k;
    float log_thr, prune_thr;
    const float *rows;  // logp of the window's first site
    float rem[kBuildMaxK + 1];
    uint32_t branch;
    std::vector<Tuple> *out;

    void walk(uint32_t d, uint32_t key, float s)
    {
        const float *lp = rows + (size_t)d * sigma;
        if (d + 1 == k) {
            for (uint32_t c = 0; c < sigma; ++c) {
                const float ns = s + lp[c];
                if (ns >= log_thr) out->push_back(Tuple{build_pack(key * sigma + c, branch), ns});
            }
            return;
        }
        for (uint32_t c = 0; c < sigma; ++c) {
            const float ns = s + lp[c];
            if (!(ns + rem[d + 1] < prune_thr)) walk(d + 1, key * sigma + c, ns);
        }
    }
};

void enumerate_ghosts(uint32_t sigma, uint32_t k, float log_thr, const float *logp, const uint32_t *branch_of, uint64_t g0,
                      uint64_t g1, uint64_t L, std::vector<Tuple> &out)
{
    Walker w;
    w.sigma = sigma, w.k = k, w.log_thr = log_thr, w.prune_thr = build_prune_threshold(log_thr, k), w.out = &out;
    std::vector<float> best(L);
    for (uint64_t g = g0; g < g1; ++g) {
        const float *node = logp + g * L * sigma;
        for (uint64_t i = 0; i < L; ++i) best[i] = *std::max_element(node + i * sigma, node + (i + 1) * sigma);
        w.branch = branch_of[g];
        for (uint64_t at = 0; at + k <= L; ++at) {
            w.rem[k] = 0.0f;
            for (uint32_t j = k; j-- > 0;) w.rem[j] = best[at + j] + w.rem[j + 1];
            w.rows = node + at * sigma;
            if (!(0.0f + w.rem[0] < w.prune_thr)) w.walk(0, 0, 0.0f);
        }
    }
}

}  // namespace

int build_check_params(uint32_t sigma, uint32_t k, uint32_t num_branches, float log_thr, std::string &err)
{
    if (sigma != 4 && sigma != 20) return invalid(err, "sigma = " + std::to_string(sigma) + " is neither 4 nor 20");
    const uint32_t max_k = sigma == 4 ? 15 : 7;
    if (k < 2 || k > max_k)
        return invalid(err, "k = " + std::to_string(k) + " is outside [2, " + std::to_string(max_k) + "] for sigma = " + std::to_string(sigma));
    if (num_branches == 0) return invalid(err, "a tree has at least one branch (num_branches is 0)");
    if (std::isnan(log_thr) || log_thr > 0.0f) return invalid(err, "log_thr must be a number that is at most 0");
    return EPIK_AMD_OK;
}

int build_check_length(uint64_t L, uint32_t k, uint64_t first_L, std::string &err)
{
    if (L < k) return invalid(err, "L = " + std::to_string(L) + " sites hold no window of k = " + std::to_string(k));
    if (L > 0xffffffffull) return invalid(err, "L = " + std::to_string(L) + " is 2^32 sites or more");
    if (first_L && L != first_L)
        return invalid(err, "L = " + std::to_string(L) + " differs from the first chunk's L = " + std::to_string(first_L));
    return EPIK_AMD_OK;
}

std::string build_bad_value(uint64_t flat, uint64_t L, uint32_t sigma, float value)
{
    const uint64_t state = flat % sigma, site = flat / sigma % L, g = flat / sigma / L;
    return "ghost node " + std::to_string(g) + ", site " + std::to_string(site) + ", state " + std::to_string(state) + ": logp is " +
           (std::isnan(value) ? std::string("NaN") : "above 0 (" + std::to_string(value) + ")");
}

std::string build_bad_branch(uint64_t g, uint32_t branch, uint32_t num_branches)
{
    return "branch_of[" + std::to_string(g) + "] = " + std::to_string(branch) + " is no branch of a tree of " + std::to_string(num_branches);
}

int build_check_chunk(const float *logp, const uint32_t *branch_of, uint64_t G, uint64_t L, uint32_t sigma,
                      uint32_t num_branches, std::string &err)
{
    if (!logp || !branch_of) return invalid(err, "null host buffer");
    const uint64_t n = G * L * sigma;
    for (uint64_t i = 0; i < n; ++i)
        if (!(logp[i] <= 0.0f)) return invalid(err, build_bad_value(i, L, sigma, logp[i]));
    for (uint64_t g = 0; g < G; ++g)
        if (branch_of[g] >= num_branches) return invalid(err, build_bad_branch(g, branch_of[g], num_branches));
    return EPIK_AMD_OK;
}

float build_prune_threshold(float log_thr, uint32_t k)
{
    const double scaled = (double)log_thr * (1.0 + 16.0 * (double)k * 0x1p-24);
    const float f = (float)scaled;
    return std::nextafter(f, -std::numeric_limits<float>::infinity());
}

int build_rule_host(uint32_t sigma, uint32_t k, float log_thr, const float *logp, const uint32_t *branch_of, uint64_t G,
                    uint64_t L, uint32_t num_threads, build_result &out, std::string &err)
{
    (void)err;
    const uint64_t threads = std::max<uint64_t>(1, std::min<uint64_t>(num_threads, G));
    std::vector<std::vector<Tuple>> parts(threads);
    if (threads == 1) {
        enumerate_ghosts(sigma, k, log_thr, logp, branch_of, 0, G, L, parts[0]);
    } else {
        std::vector<std::thread> pool;
        for (uint64_t t = 0; t < threads; ++t)
            pool.emplace_back([&, t] { enumerate_ghosts(sigma, k, log_thr, logp, branch_of, G * t / threads, G * (t + 1) / threads, L, parts[t]); });
        for (auto &th : pool) th.join();
    }
    std::vector<Tuple> all = std::move(parts[0]);
    for (uint64_t t = 1; t < threads; ++t) {
        all.insert(all.end(), parts[t].begin(), parts[t].end());
        std::vector<Tuple>().swap(parts[t]);
    }
    // best first within a (key, branch)
    std::sort(all.begin(), all.end(), [](const Tuple &a, const Tuple &b) { return a.packed != b.packed ? a.packed < b.packed : a.score > b.score; });
    out = build_result{};
    for (size_t i = 0; i < all.size(); ++i) {
        if (i && all[i].packed == all[i - 1].packed) continue;
        const uint32_t key = (uint32_t)(all[i].packed >> 32);
        if (out.keys.empty() || out.keys.back() != key) {
            if (!out.keys.empty()) out.offsets.push_back(out.values.size());
            out.keys.push_back(key);
        }
        out.values.push_back(epik_amd_pkdb_value{(uint32_t)all[i].packed, all[i].score});
    }
    if (!out.keys.empty()) out.offsets.push_back(out.values.size());
    return EPIK_AMD_OK;
}

}  // namespace epik_amd
