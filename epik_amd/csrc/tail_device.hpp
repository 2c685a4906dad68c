// tail_device.hpp -- the double-precision tail of a read's placement, a lane per reported row.
//
// place_epilogue_body (place_device.hpp) with a context that defers the tail stops behind the rank: the read's ranked
// candidates and one TailHeader lie in the launch's workspace.  What follows in the wave form -- 10^score of every
// reported row (place.cpp:254), sum_scores put together (:164-184), the LWR and filter_by_ratio (:188-199, :241-267),
// the row stores -- keeps a wave of 64 lanes busy for at most keep_at_most of them.  Here a group of kGroup lanes
// (the smallest power of two >= keep_at_most) takes a read, 64 / kGroup reads to a wave.  Every floating-point
// operation is the wave form's, on the same operands in the same order, with the same exp10: the rows are the same bytes.
#ifndef EPIK_AMD_TAIL_DEVICE_HPP
#define EPIK_AMD_TAIL_DEVICE_HPP
#include "place_device.hpp"

namespace epik_amd {
namespace {

// Lane r of the group that owns `read`; all 64 lanes of a wave call together.  active: the read exists (the groups
// behind the last read do nothing).  Reads whose header says kTailNone keep the n_rows the placement kernel wrote.
template <uint32_t kGroup>
__device__ __forceinline__ void finish_rows_group(const PlaceParams &p, const void *tail_ws, uint64_t read, uint32_t r, bool active)
{
    static_assert(kGroup >= 1 && kGroup <= 64 && (kGroup & (kGroup - 1u)) == 0, "a power of two of lanes inside a wave");
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t group_at = lane & ~(kGroup - 1u);  // the group's lane 0
    const uint32_t keep = p.keep_at_most;
    const TailHeader *headers = static_cast<const TailHeader *>(tail_ws);
    const v4u *cands = reinterpret_cast<const v4u *>(headers + p.n_reads);
    // the flags first: of the header of a read without a tail nothing else was written, and nothing else is loaded
    TailHeader h{};
    h.bits = active ? headers[read].bits : kTailNone;
    const bool none = (h.bits & kTailNone) != 0;
    if (!none) h = headers[read];
    const uint32_t n_sel = none ? 0u : (h.bits & kTailSelMask);
    const bool has_row = r < n_sel && r < keep;
    v4u cand{0u, 0u, 0u, 0u};  // {branch, score bits, k-mer count, -}
    if (has_row) cand = cands[read * keep + r];
    const bool all_underflow = (h.bits & kTailUnderflow) != 0;
    const float score = __uint_as_float(cand.y);
    // ---- 10^score of every row that will be reported (:254); the row of rank 0 carries best_score
    double my_power = 0.0;
    if (has_row && !all_underflow) my_power = pow10_f64((double)score);
    double best_power = my_power;
    float best_score = score;
    if constexpr (kGroup > 1) {
        const uint64_t bits = (uint64_t)__double_as_longlong(my_power);
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)bits, (int)group_at);
        const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(bits >> 32), (int)group_at);
        best_power = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
        best_score = __uint_as_float((uint32_t)__shfl((int)cand.y, (int)group_at));
    }
    double score_sum;
    if (h.bits & kTailRelative) {
        const double rel = h.sum;
        const double ref_power = (h.ref_score == best_score) ? best_power : pow10_f64((double)h.ref_score);
        score_sum = ref_power * rel;
    } else {
        // everything in double, term by term, as place.cpp:174-183 (the terms were summed in the wave)
        const double sum_placed = h.sum;
        score_sum = all_underflow ? 0.0 : (double)h.not_placed * pow10_f64((double)h.thr_score) + sum_placed;
    }
    const double keep_factor = (score_sum == 0.0) ? 0.0 : p.keep_factor;  // :247-251

    // ---- LWR (:241-264), filter_by_ratio (:188-199) ---------------------------------------------
    const double best_ratio =
        (score_sum == 0.0 || best_power == 0.0) ? 0.0 : best_power / score_sum;  // :191, rows[0]
    const double ratio_threshold = best_ratio * keep_factor;                      // :192
    double my_lwr = 0.0;
    if (has_row && score_sum != 0.0 && my_power != 0.0) my_lwr = my_power / score_sum;  // :255-262
    const bool kept = has_row && my_lwr >= ratio_threshold;                             // :197
    const uint64_t group_mask = kGroup == 64 ? ~0ull : (((1ull << kGroup) - 1ull) << group_at);
    const uint64_t kept_ranks = __ballot(kept) & group_mask;
    if (kept) {
        const uint32_t slot = (uint32_t)__popcll(kept_ranks & ((1ull << lane) - 1ull));
        epik_amd_placement out;
        out.branch = cand.x;
        out.score = score;
        out.lwr = my_lwr;
        p.rows[read * keep + slot] = out;
        if (p.kmer_counts) p.kmer_counts[read * keep + slot] = cand.z;
    }
    if (active && !none && r == 0) p.n_rows[read] = (uint32_t)__popcll(kept_ranks);
}

}  // namespace
}  // namespace epik_amd
#endif
