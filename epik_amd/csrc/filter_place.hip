// filter_place.hip -- ranking phylo-k-mers by informativeness: epik_amd_filter_rank_device, _filter_rank,
// _filter_rank_host, _filter_math_host and what epik_amd_builder_rank (build_place.hip) runs on a builder's device arrays
// (include/epik_amd.h, "Ranking phylo-k-mers by informativeness", where the rule is stated once; its arithmetic is
// ../host/filter.hpp, compiled here for the device and in ../host/filter.cpp for the host).
//
//   filter_value_kernel<FILTER>   a wave takes tiles of 64 consecutive keys, lane l key 64 t + l.  A lane whose list has
//                          at most 4 entries sums it by the rule's closed form; a ballot names the longer lists and the
//                          wave walks them one after the other, lane c being chain c: coalesced 8-byte loads of
//                          `values`, and per key one butterfly of lane exchanges.  Then every lane turns its own key's
//                          sums into the value: one ek_log2 per key, none per entry.  The same pass checks the offsets,
//                          scores and branches (the first offender of each kind through an atomic minimum that only an
//                          offender issues), writes the value, its sortable image and the key's index, and keeps the
//                          smallest and largest image of the call (one pair of atomics a tile).
//                          No compaction pass, no LDS, nothing read twice.
//   (hipCUB)               the stable radix sort of (image, index) over the bits in which the images differ.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <string>

#include "../host/filter.hpp"
#include "filter_entry.hpp"
#include "host_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kShortList = 4;       // lists up to this long are summed by their own lane
constexpr uint64_t kMaxBlocks = 8192;    // of four waves; the tiles beyond are strided over
constexpr uint64_t kMaxKeys = 0x7fffffffull;
enum Word : uint32_t { kBadOffset = 0, kBadScore, kBadBranch, kLowImage, kHighImage, kWords };

__device__ inline double shfl_xor_f64(double v, int mask)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, mask), hi = __shfl_xor(hi, mask);
    return __hiloint2double(hi, lo);
}

__device__ inline uint64_t shfl_u64(uint64_t v, int lane)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane);
    return (uint64_t)hi << 32 | lo;
}

__device__ inline uint64_t shfl_xor_u64(uint64_t v, int mask)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
    return (uint64_t)hi << 32 | lo;
}

// the rule's butterfly: every lane ends with a[0]
__device__ inline double butterfly_sum(double v)
{
    for (int h = kFilterChains / 2; h >= 1; h /= 2) v = v + shfl_xor_f64(v, h);
    return v;
}

// what an entry adds to its chain, with the checks
template <uint32_t FILTER>
__device__ inline void take_entry(const epik_amd_pkdb_value e, uint64_t at, uint32_t num_branches, double &a, double &b, float &best,
                                  unsigned long long *__restrict__ words)
{
    if (!(e.score <= 0.0f)) atomicMin(&words[kBadScore], (unsigned long long)at);
    if (e.branch >= num_branches) atomicMin(&words[kBadBranch], (unsigned long long)at);
    if constexpr (FILTER == EPIK_AMD_FILTER_MIF0) {
        double p, px;
        filter_terms(e.score, p, px);
        a = a + p, b = b + px;
    } else if constexpr (FILTER == EPIK_AMD_FILTER_BEST) {
        best = e.score > best ? e.score : best;
    }
}

template <uint32_t FILTER>
__global__ __launch_bounds__(kBlock) void filter_value_kernel(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ offsets,
                                                              const epik_amd_pkdb_value *__restrict__ values, uint64_t K,
                                                              uint32_t num_branches, float log_thr, uint64_t seed,
                                                              double *__restrict__ value, uint64_t *__restrict__ image,
                                                              uint32_t *__restrict__ index, unsigned long long *__restrict__ words)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t waves = (uint64_t)gridDim.x * kBlockWaves, tiles = (K + kWave - 1) / kWave, total = offsets[K];
    uint64_t low = ~0ull, high = 0;
    for (uint64_t tile = (uint64_t)blockIdx.x * kBlockWaves + threadIdx.x / kWave; tile < tiles; tile += waves) {
        const uint64_t k = tile * kWave + lane;
        const bool live = k < K;
        uint64_t lo = live ? offsets[k] : 0, hi = live ? offsets[k + 1] : 0;
        if (hi < lo || hi > total) {  // (such a list counts as empty: nothing is read through offsets that are wrong)
            atomicMin(&words[kBadOffset], (unsigned long long)k);
            lo = hi = 0;
        }
        const uint64_t n = hi - lo;
        double A = 0.0, B = 0.0;
        float best = -HUGE_VALF;
        if (n <= kShortList) {
            // the closed form: chains 0 .. 3 hold one entry each at the most, ((c0 + c2) + (c1 + c3))
            double a[kShortList], b[kShortList];
            for (uint32_t c = 0; c < kShortList; ++c) {
                a[c] = 0.0, b[c] = 0.0;
                if (c < n) take_entry<FILTER>(values[lo + c], lo + c, num_branches, a[c], b[c], best, words);
            }
            A = (a[0] + a[2]) + (a[1] + a[3]), B = (b[0] + b[2]) + (b[1] + b[3]);
        }
        // the longer lists of the tile, one after the other, the whole wave on each
        for (uint64_t todo = __ballot(n > kShortList); todo; todo &= todo - 1) {
            const int owner = __ffsll((unsigned long long)todo) - 1;
            const uint64_t first = shfl_u64(lo, owner), count = shfl_u64(n, owner);
            double a = 0.0, b = 0.0;
            float top = -HUGE_VALF;
            for (uint64_t i = lane; i < count; i += kWave) take_entry<FILTER>(values[first + i], first + i, num_branches, a, b, top, words);
            if constexpr (FILTER == EPIK_AMD_FILTER_MIF0) {
                a = butterfly_sum(a), b = butterfly_sum(b);
                if ((int)lane == owner) A = a, B = b;
            } else if constexpr (FILTER == EPIK_AMD_FILTER_BEST) {
                for (int h = kWave / 2; h >= 1; h /= 2) {
                    const float other = __shfl_xor(top, h);
                    top = other > top ? other : top;
                }
                if ((int)lane == owner) best = top;
            }
        }
        if (live) {
            double v;
            if constexpr (FILTER == EPIK_AMD_FILTER_MIF0)
                v = filter_mif0(A, B, n, num_branches, log_thr);
            else if constexpr (FILTER == EPIK_AMD_FILTER_BEST)
                v = filter_best(best, n);
            else
                v = filter_random(seed, keys[k]);
            v = filter_fold_zero(v);
            const uint64_t u = filter_image(v);
            value[k] = v, image[k] = u, index[k] = (uint32_t)k;
            low = u < low ? u : low, high = u > high ? u : high;
        }
    }
    for (int h = kWave / 2; h >= 1; h /= 2) {
        const uint64_t l = shfl_xor_u64(low, h), g = shfl_xor_u64(high, h);
        low = l < low ? l : low, high = g > high ? g : high;
    }
    if (lane == 0 && low <= high) {
        atomicMin(&words[kLowImage], (unsigned long long)low);
        atomicMax(&words[kHighImage], (unsigned long long)high);
    }
}

struct Scratch {  // (freed however the call ends, after its stream has drained)
    void *base = nullptr;
    hipStream_t stream = nullptr;
    ~Scratch()
    {
        if (!base) return;
        (void)hipStreamSynchronize(stream);
        (void)hipFree(base);
    }
};

}  // namespace

namespace epik_amd {

int filter_scratch_reserve(FilterScratch &scratch, size_t bytes, hipStream_t stream)
{
    if (bytes <= scratch.bytes) return EPIK_AMD_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    filter_scratch_free(scratch);
    HIP_TRY(hipMalloc(&scratch.base, bytes));
    scratch.bytes = bytes;
    return EPIK_AMD_OK;
}

void filter_scratch_free(FilterScratch &scratch)
{
    if (scratch.base) (void)hipFree(scratch.base);
    scratch.base = nullptr, scratch.bytes = 0;
}

int filter_rank_on_device(int device, uint32_t num_branches, float log_thr, const uint32_t *d_keys, const uint64_t *d_offsets,
                          const epik_amd_pkdb_value *d_values, uint64_t K, uint32_t filter, uint64_t seed, double *d_value,
                          uint32_t *d_order, hipStream_t stream, FilterScratch *kept)
{
    std::string err;
    if (const int rc = filter_check_params(num_branches, log_thr, filter, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
    if (K == 0) return EPIK_AMD_OK;
    if (K > kMaxKeys) return fail_with(EPIK_AMD_ERR_INVALID, "filter_rank: " + std::to_string(K) + " keys are more than 2^31 - 1");
    if (!d_keys || !d_offsets || !d_value || !d_order) return fail_with(EPIK_AMD_ERR_INVALID, "filter_rank: null device buffer");
    HIP_TRY(hipSetDevice(device));
    // one allocation: words | image | image sorted | index | hipCUB's own
    size_t cub_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr),
                                               static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), (size_t)K, 0, 64,
                                               stream));
    const uint64_t o_image = align_up(kWords * sizeof(unsigned long long)), o_sorted = o_image + align_up(K * sizeof(uint64_t));
    const uint64_t o_index = o_sorted + align_up(K * sizeof(uint64_t)), o_cub = o_index + align_up(K * sizeof(uint32_t));
    cub_bytes = std::max<size_t>(cub_bytes, 256);
    Scratch sc;  // (of this call alone, when no handle keeps one)
    sc.stream = stream;
    if (kept) {
        if (const int rc = filter_scratch_reserve(*kept, o_cub + cub_bytes, stream); rc != EPIK_AMD_OK) return rc;
    } else {
        HIP_TRY(hipMalloc(&sc.base, o_cub + cub_bytes));
    }
    uint8_t *base = static_cast<uint8_t *>(kept ? kept->base : sc.base);
    auto *words = reinterpret_cast<unsigned long long *>(base);
    auto *image = reinterpret_cast<uint64_t *>(base + o_image), *sorted = reinterpret_cast<uint64_t *>(base + o_sorted);
    auto *index = reinterpret_cast<uint32_t *>(base + o_index);
    const unsigned long long start[kWords] = {~0ull, ~0ull, ~0ull, ~0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(words, start, sizeof start, hipMemcpyHostToDevice, stream));
    const dim3 grid(grid_for((K + kWave - 1) / kWave, kMaxBlocks)), block(kBlock);
    if (filter == EPIK_AMD_FILTER_MIF0)
        hipLaunchKernelGGL(filter_value_kernel<EPIK_AMD_FILTER_MIF0>, grid, block, 0, stream, d_keys, d_offsets, d_values, K, num_branches,
                           log_thr, seed, d_value, image, index, words);
    else if (filter == EPIK_AMD_FILTER_BEST)
        hipLaunchKernelGGL(filter_value_kernel<EPIK_AMD_FILTER_BEST>, grid, block, 0, stream, d_keys, d_offsets, d_values, K, num_branches,
                           log_thr, seed, d_value, image, index, words);
    else
        hipLaunchKernelGGL(filter_value_kernel<EPIK_AMD_FILTER_RANDOM>, grid, block, 0, stream, d_keys, d_offsets, d_values, K, num_branches,
                           log_thr, seed, d_value, image, index, words);
    HIP_TRY(hipGetLastError());
    unsigned long long found[kWords];
    HIP_TRY(hipMemcpyAsync(found, words, sizeof found, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (found[kBadOffset] != ~0ull) {
        uint64_t pair[2], total = 0;
        HIP_TRY(hipMemcpy(pair, d_offsets + found[kBadOffset], sizeof pair, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&total, d_offsets + K, sizeof total, hipMemcpyDeviceToHost));
        return fail_with(EPIK_AMD_ERR_INVALID, filter_bad_offsets(found[kBadOffset], pair[0], pair[1], total));
    }
    for (const Word kind : {kBadScore, kBadBranch})
        if (found[kind] != ~0ull) {
            epik_amd_pkdb_value e{};
            HIP_TRY(hipMemcpy(&e, d_values + found[kind], sizeof e, hipMemcpyDeviceToHost));
            return fail_with(EPIK_AMD_ERR_INVALID, kind == kBadScore ? filter_bad_score(found[kind], e.score)
                                                                      : filter_bad_branch(found[kind], e.branch, num_branches));
        }
    // only the bits in which the images differ are sorted: all of them share what stands above the highest such bit
    const uint64_t differ = found[kLowImage] ^ found[kHighImage];
    if (differ == 0) {
        HIP_TRY(hipMemcpyAsync(d_order, index, K * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    } else {
        const int end_bit = 64 - __builtin_clzll(differ);
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(base + o_cub, cub_bytes, image, sorted, index, d_order, (size_t)K, 0, end_bit, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return EPIK_AMD_OK;
}

}  // namespace epik_amd

extern "C" {

int epik_amd_filter_rank_device(int device, uint32_t num_branches, float log_thr, const void *d_keys, const void *d_offsets,
                                const void *d_values, uint64_t K, uint32_t filter, uint64_t seed, void *d_value, void *d_order,
                                void *stream)
{
    try {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail_with(EPIK_AMD_ERR_NO_DEVICE, "no HIP device");
        if (device < 0 || device >= count) return fail_with(EPIK_AMD_ERR_INVALID, "device " + std::to_string(device) + " does not exist");
        return filter_rank_on_device(device, num_branches, log_thr, static_cast<const uint32_t *>(d_keys),
                                     static_cast<const uint64_t *>(d_offsets), static_cast<const epik_amd_pkdb_value *>(d_values), K, filter,
                                     seed, static_cast<double *>(d_value), static_cast<uint32_t *>(d_order), static_cast<hipStream_t>(stream));
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("filter_rank_device: ") + e.what());
    }
}

int epik_amd_filter_rank(int device, uint32_t num_branches, float log_thr, const uint32_t *keys, const uint64_t *offsets,
                         const epik_amd_pkdb_value *values, uint64_t K, uint32_t filter, uint64_t seed, double *value, uint32_t *order)
{
    try {
        std::string err;
        if (const int rc = filter_check_params(num_branches, log_thr, filter, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        if (K == 0) return EPIK_AMD_OK;
        if (!keys || !offsets || !value || !order) return fail_with(EPIK_AMD_ERR_INVALID, "filter_rank: null host buffer");
        // (the device reads values through offsets it has checked against offsets[K]: the upload must hold that many)
        for (uint64_t k = 0; k < K; ++k)
            if (offsets[k + 1] < offsets[k]) return fail_with(EPIK_AMD_ERR_INVALID, filter_bad_offsets(k, offsets[k], offsets[k + 1], offsets[K]));
        const uint64_t E = offsets[K];
        if (E && !values) return fail_with(EPIK_AMD_ERR_INVALID, "filter_rank: null host buffer");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail_with(EPIK_AMD_ERR_NO_DEVICE, "no HIP device");
        if (device < 0 || device >= count) return fail_with(EPIK_AMD_ERR_INVALID, "device " + std::to_string(device) + " does not exist");
        HIP_TRY(hipSetDevice(device));
        const uint64_t o_offsets = align_up(K * sizeof(uint32_t)), o_values = o_offsets + align_up((K + 1) * sizeof(uint64_t));
        const uint64_t o_value = o_values + align_up(E * sizeof(epik_amd_pkdb_value)), o_order = o_value + align_up(K * sizeof(double));
        Scratch up;
        HIP_TRY(hipMalloc(&up.base, o_order + align_up(K * sizeof(uint32_t))));
        uint8_t *base = static_cast<uint8_t *>(up.base);
        HIP_TRY(hipMemcpy(base, keys, K * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(base + o_offsets, offsets, (K + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        if (E) HIP_TRY(hipMemcpy(base + o_values, values, E * sizeof(epik_amd_pkdb_value), hipMemcpyHostToDevice));
        if (const int rc = filter_rank_on_device(device, num_branches, log_thr, reinterpret_cast<const uint32_t *>(base),
                                                 reinterpret_cast<const uint64_t *>(base + o_offsets),
                                                 reinterpret_cast<const epik_amd_pkdb_value *>(base + o_values), K, filter, seed,
                                                 reinterpret_cast<double *>(base + o_value), reinterpret_cast<uint32_t *>(base + o_order),
                                                 nullptr);
            rc != EPIK_AMD_OK)
            return rc;
        HIP_TRY(hipMemcpy(value, base + o_value, K * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(order, base + o_order, K * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("filter_rank: ") + e.what());
    }
}

int epik_amd_filter_rank_host(uint32_t num_branches, float log_thr, const uint32_t *keys, const uint64_t *offsets,
                              const epik_amd_pkdb_value *values, uint64_t K, uint32_t filter, uint64_t seed, uint32_t num_threads,
                              double *value, uint32_t *order)
{
    try {
        if (K && (!keys || !offsets || !value || !order || (offsets[K] && !values)))
            return fail_with(EPIK_AMD_ERR_INVALID, "filter_rank: null host buffer");
        std::string err;
        if (const int rc = filter_rank_host(num_branches, log_thr, keys, offsets, values, K, filter, seed, num_threads, value, order, err);
            rc != EPIK_AMD_OK)
            return fail_with(rc, err);
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("filter_rank_host: ") + e.what());
    }
}

int epik_amd_filter_math_host(const double *x, uint64_t n, double *exp2_out, double *log2_out)
{
    if (n && !x) return fail_with(EPIK_AMD_ERR_INVALID, "filter_math_host: null argument");
    filter_math_host(x, n, exp2_out, log2_out);
    return EPIK_AMD_OK;
}

}  // extern "C"
