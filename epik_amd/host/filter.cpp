// filter.cpp -- ranking phylo-k-mers by informativeness on the host (include/epik_amd.h, "Ranking phylo-k-mers by
// informativeness"): what epik_amd_filter_rank_host and epik_amd_filter_math_host run, and the checks and messages that
// the device path (csrc/filter_place.hip) shares.  Plain C++, no device.
#include "filter.hpp"

#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "parallel.hpp"

namespace epik_amd {

namespace {

constexpr uint64_t kKeysPerItem = 4096;  // keys a thread takes at a time
constexpr uint64_t kNone = ~0ull;

std::string number(float v)
{
    char text[40];
    std::snprintf(text, sizeof text, "%.9g", (double)v);
    return text;
}

// the 64 interleaved chains of the rule, combined by its butterfly
double chained_sum(double *chain)
{
    for (uint32_t h = kFilterChains / 2; h >= 1; h /= 2)
        for (uint32_t c = 0; c < h; ++c) chain[c] += chain[c + h];
    return chain[0];
}

double value_of_key(uint32_t num_branches, float log_thr, uint32_t key, const epik_amd_pkdb_value *list, uint64_t n, uint32_t filter,
                    uint64_t seed)
{
    if (filter == EPIK_AMD_FILTER_RANDOM) return filter_random(seed, key);
    if (filter == EPIK_AMD_FILTER_BEST) {
        float best = n ? list[0].score : 0.0f;
        for (uint64_t i = 1; i < n; ++i) best = list[i].score > best ? list[i].score : best;
        return filter_best(best, n);
    }
    double a[kFilterChains], b[kFilterChains];
    for (uint32_t c = 0; c < kFilterChains; ++c) a[c] = 0.0, b[c] = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        double p, px;
        filter_terms(list[i].score, p, px);
        a[i % kFilterChains] += p;
        b[i % kFilterChains] += px;
    }
    const double A = chained_sum(a), B = chained_sum(b);
    return filter_mif0(A, B, n, num_branches, log_thr);
}

}  // namespace

int filter_check_params(uint32_t num_branches, float log_thr, uint32_t filter, std::string &err)
{
    if (filter != EPIK_AMD_FILTER_BEST && filter != EPIK_AMD_FILTER_MIF0 && filter != EPIK_AMD_FILTER_RANDOM) {
        err = "filter_rank: unknown filter " + std::to_string(filter) + " (0 best, 1 mif0, 2 random)";
        return EPIK_AMD_ERR_INVALID;
    }
    if (num_branches < 1) {
        err = "filter_rank: num_branches must be at least 1";
        return EPIK_AMD_ERR_INVALID;
    }
    if (!(log_thr <= 0.0f)) {
        err = "filter_rank: log_thr = " + number(log_thr) + " must be at most 0";
        return EPIK_AMD_ERR_INVALID;
    }
    return EPIK_AMD_OK;
}

std::string filter_bad_offsets(uint64_t k, uint64_t lo, uint64_t hi, uint64_t total)
{
    if (hi < lo)
        return "filter_rank: offsets are not ascending: offsets[" + std::to_string(k + 1) + "] = " + std::to_string(hi) + " is below offsets[" +
               std::to_string(k) + "] = " + std::to_string(lo);
    return "filter_rank: offsets are not ascending: offsets[" + std::to_string(k + 1) + "] = " + std::to_string(hi) +
           " is above the last one, " + std::to_string(total);
}

std::string filter_bad_score(uint64_t i, float score)
{
    return "filter_rank: values[" + std::to_string(i) + "].score = " + number(score) + " is a NaN or above 0";
}

std::string filter_bad_branch(uint64_t i, uint32_t branch, uint32_t num_branches)
{
    return "filter_rank: values[" + std::to_string(i) + "].branch = " + std::to_string(branch) + " is not below num_branches = " +
           std::to_string(num_branches);
}

int filter_rank_host(uint32_t num_branches, float log_thr, const uint32_t *keys, const uint64_t *offsets,
                     const epik_amd_pkdb_value *values, uint64_t K, uint32_t filter, uint64_t seed, uint32_t num_threads,
                     double *value, uint32_t *order, std::string &err)
{
    if (const int rc = filter_check_params(num_branches, log_thr, filter, err); rc != EPIK_AMD_OK) return rc;
    if (K == 0) return EPIK_AMD_OK;
    if (K > 0xffffffffull) {
        err = "filter_rank: " + std::to_string(K) + " keys do not fit an order of uint32";
        return EPIK_AMD_ERR_INVALID;
    }
    const uint64_t items = (K + kKeysPerItem - 1) / kKeysPerItem, total = offsets[K];
    // the first offender of every kind, per item; a list with bad offsets counts as empty
    std::vector<uint64_t> bad_offset(items, kNone), bad_score(items, kNone), bad_branch(items, kNone);
    std::vector<std::pair<uint64_t, uint32_t>> image(K);
    parallel_for(items, num_threads, [&](size_t item) {
        const uint64_t k1 = std::min<uint64_t>(K, (item + 1) * kKeysPerItem);
        for (uint64_t k = item * kKeysPerItem; k < k1; ++k) {
            uint64_t lo = offsets[k], hi = offsets[k + 1];
            if (hi < lo || hi > total) {
                if (bad_offset[item] == kNone) bad_offset[item] = k;
                hi = lo = 0;
            }
            for (uint64_t i = lo; i < hi; ++i) {
                if (!(values[i].score <= 0.0f) && bad_score[item] == kNone) bad_score[item] = i;
                if (values[i].branch >= num_branches && bad_branch[item] == kNone) bad_branch[item] = i;
            }
            const double v = filter_fold_zero(value_of_key(num_branches, log_thr, keys[k], values + lo, hi - lo, filter, seed));
            value[k] = v;
            image[k] = {filter_image(v), (uint32_t)k};
        }
    });
    const auto first = [](const std::vector<uint64_t> &found) {
        for (const uint64_t at : found)
            if (at != kNone) return at;
        return kNone;
    };
    if (const uint64_t k = first(bad_offset); k != kNone) {
        err = filter_bad_offsets(k, offsets[k], offsets[k + 1], total);
        return EPIK_AMD_ERR_INVALID;
    }
    if (const uint64_t i = first(bad_score); i != kNone) {
        err = filter_bad_score(i, values[i].score);
        return EPIK_AMD_ERR_INVALID;
    }
    if (const uint64_t i = first(bad_branch); i != kNone) {
        err = filter_bad_branch(i, values[i].branch, num_branches);
        return EPIK_AMD_ERR_INVALID;
    }
    // (image, index) pairs are all different: sorted runs merged pairwise give the one order there is
    uint64_t runs = 1;
    while (runs < num_threads && runs < 64 && K / (runs * 2) >= 4096) runs *= 2;
    const uint64_t per_run = (K + runs - 1) / runs;
    const auto bound = [&](uint64_t r) { return std::min<uint64_t>(K, r * per_run); };
    parallel_for(runs, num_threads, [&](size_t r) { std::sort(image.begin() + bound(r), image.begin() + bound(r + 1)); });
    for (uint64_t width = 1; width < runs; width *= 2)
        parallel_for(runs / (2 * width), num_threads, [&](size_t pair) {
            const uint64_t r = pair * 2 * width;
            std::inplace_merge(image.begin() + bound(r), image.begin() + bound(r + width), image.begin() + bound(r + 2 * width));
        });
    for (uint64_t k = 0; k < K; ++k) order[k] = image[k].second;
    return EPIK_AMD_OK;
}

void filter_math_host(const double *x, uint64_t n, double *exp2_out, double *log2_out)
{
    for (uint64_t i = 0; i < n; ++i) {
        if (exp2_out) exp2_out[i] = ek_exp2(x[i]);
        if (log2_out) log2_out[i] = ek_log2(x[i]);
    }
}

}  // namespace epik_amd
