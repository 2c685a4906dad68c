// build_place.hip -- phylo-k-mer databases built from ancestral posteriors: epik_amd_builder_create, _add,
// _add_device, _finish, _copy, _rank, _destroy and epik_amd_build_host (include/epik_amd.h, where the rule is stated once;
// _rank hands the finished arrays to filter_place.hip).
//
// The reference's world builds its databases in another product on CPU threads (IPK); nothing of it is restated here.
//
// A chunk of ghost nodes goes through
//   validate_kernel        (add_device only) the first NaN or value above 0, the first branch_of[g] >= N;
//   enumerate_kernel<.,0>  the survivors of every (ghost node, window, first letter), counted;
//   (hipCUB)               the exclusive sum of the counts: where every item's survivors go, and how many there are;
//   enumerate_kernel<.,1>  the same walk again, every survivor written at its own place: (key, branch) packed in one
//                          word, and the score;
//   (hipCUB)               the radix sort of the tuples by that word;
//   head_flag_kernel, (hipCUB) sum, reduce_kernel    one tuple per (key, branch), the best score of its run;
//   merge_rank_kernel, (hipCUB) sum, merge_write_kernel    the chunk merged into the running store, itself sorted
//                          and without repeats: a score of a pair the store has is raised in place, the new pairs and the
//                          old ones are written to the next store at their ranks.
// The walk.  A workgroup takes a tile of 64 windows of one ghost node and stages its (64 + k - 1) x sigma logp values in
// LDS, with the best letter of every site and, per window and depth, the sum of the best remaining letters.  Every lane
// owns the subtree below one (window, first letter) and walks it depth first: its state is a depth, the key so far and
// a stack of at most k - 2 prefix sums in LDS, whatever the number of survivors -- nothing on chip can overflow, and
// the count pass sizes global memory exactly before the fill pass writes.  (Level-by-level expansion with ballot
// compaction would need a frontier whose size nothing bounds below sigma^k per window.)
// finish: head_flag_kernel on the keys of the store, a sum, and csr_kernel.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../host/build.hpp"
#include "../host/filter.hpp"
#include "filter_entry.hpp"
#include "host_entry.hpp"

struct epik_amd_builder {
    int device = -1;  // -1: the finished result of epik_amd_build_host
    uint32_t sigma = 0, k = 0, num_branches = 0, branch_bits = 0, key_bits = 0;
    float log_thr = 0, prune_thr = 0;
    uint64_t L = 0;  // of the first chunk (0: none yet)
    uint64_t ws_bytes = 0, splits = 0;
    uint8_t *ws = nullptr;
    void *temp = nullptr;
    size_t temp_bytes = 0;
    unsigned long long *d_words = nullptr;  // two words the kernels report through
    hipStream_t stream = nullptr;
    // the running store: (key << branch_bits | branch) ascending without repeats, and the scores
    uint64_t *store_packed = nullptr;
    float *store_score = nullptr;
    uint64_t store_n = 0;
    // the finished result
    bool finished = false;
    uint64_t num_keys = 0, num_entries = 0;
    uint32_t *d_keys = nullptr;
    uint64_t *d_offsets = nullptr;
    epik_amd_pkdb_value *d_values = nullptr;
    epik_amd::build_result host;
    // what builder_rank keeps between calls: the ranking's scratch, and value | order of the last call
    epik_amd::FilterScratch rank_scratch, rank_out;
};

namespace {

using namespace epik_amd;

constexpr uint32_t kTile = 64, kMaxRows = kTile + kBuildMaxK - 1;
constexpr uint64_t kMaxBlocks = 16384;
constexpr uint64_t kTupleBytes = 4 * sizeof(uint64_t) + 2 * sizeof(float);  // four words and two scores a tuple
constexpr uint64_t kMaxTuples = 0x7fffffffull;
static_assert(sizeof(epik_amd_pkdb_value) == 8 && kTile <= kBlock);

uint32_t bits_for(uint64_t values)  // bits that hold 0 .. values - 1
{
    uint32_t b = 1;
    while (b < 64 && (1ull << b) < values) ++b;
    return b;
}

uint32_t blocks_for(uint64_t threads) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((threads + kBlock - 1) / kBlock, kMaxBlocks)); }

// ---- kernels ----------------------------------------------------------------------------------------------------

// words[0]: the smallest flat index of a logp value that is NaN or above 0; words[1]: the smallest g with branch_of[g] >= N
__global__ __launch_bounds__(kBlock) void validate_kernel(const float *__restrict__ logp, uint64_t n, const uint32_t *__restrict__ branch_of,
                                                          uint64_t G, uint32_t num_branches, unsigned long long *__restrict__ words)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, first = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    for (uint64_t i = first; i < n; i += stride)
        if (!(logp[i] <= 0.0f)) atomicMin(&words[0], (unsigned long long)i);
    for (uint64_t g = first; g < G; g += stride)
        if (branch_of[g] >= num_branches) atomicMin(&words[1], (unsigned long long)g);
}

// Item ((g * W) + w) * SIGMA + c0 of the chunk's n_ghosts ghost nodes from g_begin on: the survivors among the k-mers of
// window w that start with c0.  FILL = false: counts[item]; FILL = true: survivor number n of the item goes to
// offs[item] + n (nothing is written at or beyond `cap`).
template <uint32_t SIGMA, bool FILL>
__global__ __launch_bounds__(kBlock) void enumerate_kernel(const float *__restrict__ logp, const uint32_t *__restrict__ branch_of,
                                                           uint64_t g_begin, uint64_t n_ghosts, uint32_t L, uint32_t k, float log_thr,
                                                           float prune_thr, uint32_t branch_bits, uint64_t *__restrict__ counts,
                                                           const uint64_t *__restrict__ offs, uint64_t cap,
                                                           uint64_t *__restrict__ packed, float *__restrict__ scores)
{
    __shared__ float s_logp[kMaxRows * SIGMA];
    __shared__ float s_best[kMaxRows];
    __shared__ float s_rem[(kBuildMaxK + 1) * kTile];
    __shared__ float s_stack[kBuildMaxK * kBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t W = L - k + 1, tiles = (W + kTile - 1) / kTile;
    const uint64_t units = n_ghosts * tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint64_t gl = u / tiles;
        const uint32_t w0 = (uint32_t)(u % tiles) * kTile;
        const uint32_t nwin = min(kTile, W - w0), rows = nwin + k - 1;
        const float *node = logp + ((g_begin + gl) * L + w0) * SIGMA;
        __syncthreads();  // (the tile before is read no more)
        for (uint32_t i = tid; i < rows * SIGMA; i += kBlock) s_logp[i] = node[i];
        __syncthreads();
        for (uint32_t r = tid; r < rows; r += kBlock) {
            float m = s_logp[r * SIGMA];
#pragma unroll
            for (uint32_t c = 1; c < SIGMA; ++c) m = fmaxf(m, s_logp[r * SIGMA + c]);
            s_best[r] = m;
        }
        __syncthreads();
        if (tid < nwin) {  // s_rem[d][t]: the best letters of positions d .. k - 1 of window t, summed from the right
            float r = 0.0f;
            s_rem[k * kTile + tid] = r;
            for (uint32_t j = k; j-- > 0;) {
                r = s_best[tid + j] + r;
                s_rem[j * kTile + tid] = r;
            }
        }
        __syncthreads();
        const uint32_t branch = branch_of[g_begin + gl];
        for (uint32_t item = tid; item < nwin * SIGMA; item += kBlock) {
            const uint32_t t = item / SIGMA, c0 = item % SIGMA;
            const uint64_t gi = (gl * W + w0 + t) * SIGMA + c0;
            const uint64_t base = FILL ? offs[gi] : 0;
            uint64_t n = 0;
            float s = 0.0f + s_logp[t * SIGMA + c0];
            if (!(s + s_rem[kTile + t] < prune_thr)) {
                uint32_t d = 1, key = c0, c = 0;  // d letters chosen, their sum s; c: the next letter to try at position d
                while (true) {
                    if (d + 1 == k) {  // the leaves below this prefix: the exact test
                        const float *lp = s_logp + (t + d) * SIGMA;
#pragma unroll
                        for (uint32_t cc = 0; cc < SIGMA; ++cc) {
                            const float ns = s + lp[cc];
                            if (ns >= log_thr) {
                                if (FILL) {
                                    const uint64_t pos = base + n;
                                    if (pos < cap) {
                                        packed[pos] = (uint64_t)(key * SIGMA + cc) << branch_bits | branch;
                                        scores[pos] = ns;
                                    }
                                }
                                ++n;
                            }
                        }
                        c = SIGMA;
                    }
                    bool down = false;
                    while (c < SIGMA) {
                        const float ns = s + s_logp[(t + d) * SIGMA + c];
                        if (!(ns + s_rem[(d + 1) * kTile + t] < prune_thr)) {
                            s_stack[(d - 1) * kBlock + tid] = s;
                            key = key * SIGMA + c, s = ns, ++d, c = 0;
                            down = true;
                            break;
                        }
                        ++c;
                    }
                    if (down) continue;
                    if (d == 1) break;
                    --d;
                    c = key % SIGMA + 1, key /= SIGMA;
                    s = s_stack[(d - 1) * kBlock + tid];
                }
            }
            if (!FILL) counts[gi] = n;
        }
    }
}

// flags[i] = 1 where word i >> shift differs from the one before (i = 0: 1); flags[n] = 0
__global__ __launch_bounds__(kBlock) void head_flag_kernel(const uint64_t *__restrict__ words, uint64_t n, uint32_t shift,
                                                           uint64_t *__restrict__ flags)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kBlock)
        flags[i] = i == n ? 0 : (i == 0 || (words[i] >> shift) != (words[i - 1] >> shift)) ? 1 : 0;
}

// pos = the exclusive sum of head flags over n + 1 slots: tuple i belongs to run pos[i + 1] - 1.  The run's word goes out
// once; its best score by an atomic minimum over the scores' bit patterns -- scores are <= 0 and never -0.0, so the
// smaller pattern is the larger float -- which no order of arrival changes.  out_bits starts as all ones.
__global__ __launch_bounds__(kBlock) void reduce_kernel(const uint64_t *__restrict__ words, const float *__restrict__ scores,
                                                        const uint64_t *__restrict__ pos, uint64_t n, uint64_t *__restrict__ out_words,
                                                        uint32_t *__restrict__ out_bits)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t slot = pos[i + 1] - 1;
        if (pos[i + 1] != pos[i]) out_words[slot] = words[i];
        atomicMin(&out_bits[slot], __float_as_uint(scores[i]));
    }
}

// the number of words of a[0 .. n) below x
__device__ inline uint64_t lower_bound(const uint64_t *__restrict__ a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Chunk pair j against the store: rank[j] = the store's pairs below it; a pair the store has raises that score in place
// (one writer: the chunk has no repeats) and is no new pair.  is_new has nb + 1 slots, the last one 0.
__global__ __launch_bounds__(kBlock) void merge_rank_kernel(const uint64_t *__restrict__ a_words, float *__restrict__ a_scores, uint64_t na,
                                                            const uint64_t *__restrict__ b_words, const float *__restrict__ b_scores,
                                                            uint64_t nb, uint64_t *__restrict__ rank, uint64_t *__restrict__ is_new)
{
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= nb; j += (uint64_t)gridDim.x * kBlock) {
        if (j == nb) {
            is_new[j] = 0;
            continue;
        }
        const uint64_t r = lower_bound(a_words, na, b_words[j]);
        const bool have = r < na && a_words[r] == b_words[j];
        if (have && b_scores[j] > a_scores[r]) a_scores[r] = b_scores[j];
        rank[j] = r;
        is_new[j] = have ? 0 : 1;
    }
}

// new_pos = the exclusive sum of is_new.  Store pair i goes to i + the new pairs below it, new pair j to rank[j] + new_pos[j].
__global__ __launch_bounds__(kBlock) void merge_write_kernel(const uint64_t *__restrict__ a_words, const float *__restrict__ a_scores, uint64_t na,
                                                             const uint64_t *__restrict__ b_words, const float *__restrict__ b_scores,
                                                             uint64_t nb, const uint64_t *__restrict__ rank,
                                                             const uint64_t *__restrict__ new_pos, uint64_t n_out,
                                                             uint64_t *__restrict__ out_words, float *__restrict__ out_scores)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < na + nb; i += (uint64_t)gridDim.x * kBlock) {
        uint64_t at, word;
        float score;
        if (i < na) {
            word = a_words[i], score = a_scores[i];
            at = i + new_pos[lower_bound(b_words, nb, word)];
        } else {
            const uint64_t j = i - na;
            if (new_pos[j + 1] == new_pos[j]) continue;
            word = b_words[j], score = b_scores[j];
            at = rank[j] + new_pos[j];
        }
        if (at < n_out) out_words[at] = word, out_scores[at] = score;
    }
}

// the store as CSR: pos = the exclusive sum of the head flags of the keys
__global__ __launch_bounds__(kBlock) void csr_kernel(const uint64_t *__restrict__ words, const float *__restrict__ scores,
                                                     const uint64_t *__restrict__ pos, uint64_t n, uint32_t branch_bits, uint64_t num_keys,
                                                     uint32_t *__restrict__ keys, uint64_t *__restrict__ offsets,
                                                     epik_amd_pkdb_value *__restrict__ values)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kBlock) {
        if (i == n) {
            offsets[num_keys] = n;
            continue;
        }
        const uint64_t word = words[i];
        if (pos[i + 1] != pos[i] && pos[i] < num_keys) keys[pos[i]] = (uint32_t)(word >> branch_bits), offsets[pos[i]] = i;
        values[i] = epik_amd_pkdb_value{(uint32_t)(word & ((1ull << branch_bits) - 1)), scores[i]};
    }
}

// ---- host side --------------------------------------------------------------------------------------------------

int ensure_temp(epik_amd_builder *b, size_t bytes)
{
    if (bytes <= b->temp_bytes) return EPIK_AMD_OK;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (b->temp) HIP_TRY(hipFree(b->temp));
    b->temp = nullptr, b->temp_bytes = 0;
    HIP_TRY(hipMalloc(&b->temp, bytes));
    b->temp_bytes = bytes;
    return EPIK_AMD_OK;
}

// the exclusive sum of n words on the builder's stream
int exclusive_sum(epik_amd_builder *b, const uint64_t *in, uint64_t *out, uint64_t n)
{
    size_t bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (size_t)n, b->stream));
    if (const int rc = ensure_temp(b, std::max<size_t>(bytes, 256)); rc != EPIK_AMD_OK) return rc;
    bytes = b->temp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b->temp, bytes, in, out, (size_t)n, b->stream));
    return EPIK_AMD_OK;
}

int read_word(epik_amd_builder *b, const uint64_t *d_word, uint64_t &value)
{
    HIP_TRY(hipMemcpyAsync(&value, d_word, sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return EPIK_AMD_OK;
}

template <bool FILL>
void launch_enumerate(epik_amd_builder *b, const float *d_logp, const uint32_t *d_branch_of, uint64_t g_begin, uint64_t n_ghosts,
                      uint64_t *counts, const uint64_t *offs, uint64_t cap, uint64_t *packed, float *scores)
{
    const uint32_t L = (uint32_t)b->L, tiles = (L - b->k + 1 + kTile - 1) / kTile;
    const dim3 grid((uint32_t)std::min<uint64_t>(n_ghosts * tiles, 1u << 20));
    if (b->sigma == 4)
        hipLaunchKernelGGL((enumerate_kernel<4, FILL>), grid, dim3(kBlock), 0, b->stream, d_logp, d_branch_of, g_begin, n_ghosts, L, b->k,
                           b->log_thr, b->prune_thr, b->branch_bits, counts, offs, cap, packed, scores);
    else
        hipLaunchKernelGGL((enumerate_kernel<20, FILL>), grid, dim3(kBlock), 0, b->stream, d_logp, d_branch_of, g_begin, n_ghosts, L, b->k,
                           b->log_thr, b->prune_thr, b->branch_bits, counts, offs, cap, packed, scores);
}

// the chunk's pairs (nb of them, sorted, no repeats) into the store
int merge_into_store(epik_amd_builder *b, const uint64_t *b_words, const float *b_scores, uint64_t nb, uint64_t *rank, uint64_t *is_new,
                     uint64_t *new_pos)
{
    hipLaunchKernelGGL(merge_rank_kernel, dim3(blocks_for(nb + 1)), dim3(kBlock), 0, b->stream, b->store_packed, b->store_score,
                       b->store_n, b_words, b_scores, nb, rank, is_new);
    HIP_TRY(hipGetLastError());
    if (const int rc = exclusive_sum(b, is_new, new_pos, nb + 1); rc != EPIK_AMD_OK) return rc;
    uint64_t n_new = 0;
    if (const int rc = read_word(b, new_pos + nb, n_new); rc != EPIK_AMD_OK) return rc;
    if (n_new == 0) return EPIK_AMD_OK;
    const uint64_t n_out = b->store_n + n_new;
    uint64_t *out_words = nullptr;
    float *out_scores = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&out_words), n_out * sizeof(uint64_t)));
    if (const hipError_t e = hipMalloc(reinterpret_cast<void **>(&out_scores), n_out * sizeof(float)); e != hipSuccess) {
        (void)hipFree(out_words);
        return fail_with(EPIK_AMD_ERR_HIP, std::string("hipMalloc of the store: ") + hipGetErrorString(e));
    }
    hipLaunchKernelGGL(merge_write_kernel, dim3(blocks_for(b->store_n + nb)), dim3(kBlock), 0, b->stream, b->store_packed, b->store_score,
                       b->store_n, b_words, b_scores, nb, rank, new_pos, n_out, out_words, out_scores);
    const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(b->stream);
    if (launched != hipSuccess || done != hipSuccess) {
        (void)hipFree(out_words), (void)hipFree(out_scores);
        return fail_with(EPIK_AMD_ERR_HIP, std::string("merge into the store: ") + hipGetErrorString(launched != hipSuccess ? launched : done));
    }
    if (b->store_packed) (void)hipFree(b->store_packed);
    if (b->store_score) (void)hipFree(b->store_score);
    b->store_packed = out_words, b->store_score = out_scores, b->store_n = n_out;
    return EPIK_AMD_OK;
}

// Ghost nodes [g0, g1) of a checked chunk on the device.  *too_large = true (and EPIK_AMD_OK): they do not fit the
// workspace, nothing was added, *need_bytes says what they take.
int add_range(epik_amd_builder *b, const float *d_logp, const uint32_t *d_branch_of, uint64_t g0, uint64_t g1, bool *too_large,
              uint64_t *need_bytes)
{
    *too_large = false;
    const uint64_t W = b->L - b->k + 1, items = (g1 - g0) * W * b->sigma;
    const uint64_t item_bytes = align_up((items + 1) * sizeof(uint64_t));
    const uint64_t slack = 8 * 256;
    *need_bytes = 2 * item_bytes + slack + kTupleBytes;
    if (*need_bytes > b->ws_bytes) {
        *too_large = true;
        return EPIK_AMD_OK;
    }
    auto *counts = reinterpret_cast<uint64_t *>(b->ws), *offs = reinterpret_cast<uint64_t *>(b->ws + item_bytes);
    const uint64_t cap = std::min<uint64_t>((b->ws_bytes - 2 * item_bytes - slack) / kTupleBytes, kMaxTuples);
    HIP_TRY(hipMemsetAsync(counts, 0, (items + 1) * sizeof(uint64_t), b->stream));
    launch_enumerate<false>(b, d_logp, d_branch_of, g0, g1 - g0, counts, nullptr, 0, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    if (const int rc = exclusive_sum(b, counts, offs, items + 1); rc != EPIK_AMD_OK) return rc;
    uint64_t total = 0;
    if (const int rc = read_word(b, offs + items, total); rc != EPIK_AMD_OK) return rc;
    if (total == 0) return EPIK_AMD_OK;
    if (total > cap) {
        *too_large = true;
        *need_bytes = 2 * item_bytes + slack + total * kTupleBytes;
        return EPIK_AMD_OK;
    }
    // four word buffers of cap + 1 and two score buffers of cap behind the items' arrays
    // (4 align_up(8 (cap + 1)) + 8 cap <= 40 cap + 1052: `slack` covers the rest)
    const uint64_t word_bytes = align_up((cap + 1) * sizeof(uint64_t));
    uint8_t *at = b->ws + 2 * item_bytes;
    uint64_t *p[4];
    for (auto &buf : p) buf = reinterpret_cast<uint64_t *>(at), at += word_bytes;
    float *s0 = reinterpret_cast<float *>(at), *s1 = s0 + cap;
    launch_enumerate<true>(b, d_logp, d_branch_of, g0, g1 - g0, nullptr, offs, total, p[0], s0);
    HIP_TRY(hipGetLastError());
    hipcub::DoubleBuffer<uint64_t> words(p[0], p[1]);
    hipcub::DoubleBuffer<float> scores(s0, s1);
    const int end_bit = (int)(b->branch_bits + b->key_bits);
    size_t bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, words, scores, (int)total, 0, end_bit, b->stream));
    if (const int rc = ensure_temp(b, std::max<size_t>(bytes, 256)); rc != EPIK_AMD_OK) return rc;
    bytes = b->temp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(b->temp, bytes, words, scores, (int)total, 0, end_bit, b->stream));
    uint64_t *sorted = words.Current(), *spare = words.Alternate();
    float *sorted_scores = scores.Current(), *spare_scores = scores.Alternate();
    // one pair per (key, branch): flags in `spare`, their sum in p[2], the pairs in p[3] and spare_scores
    hipLaunchKernelGGL(head_flag_kernel, dim3(blocks_for(total + 1)), dim3(kBlock), 0, b->stream, sorted, total, 0u, spare);
    HIP_TRY(hipGetLastError());
    if (const int rc = exclusive_sum(b, spare, p[2], total + 1); rc != EPIK_AMD_OK) return rc;
    uint64_t nb = 0;
    if (const int rc = read_word(b, p[2] + total, nb); rc != EPIK_AMD_OK) return rc;
    HIP_TRY(hipMemsetAsync(spare_scores, 0xff, nb * sizeof(float), b->stream));
    hipLaunchKernelGGL(reduce_kernel, dim3(blocks_for(total)), dim3(kBlock), 0, b->stream, sorted, sorted_scores, p[2], total, p[3],
                       reinterpret_cast<uint32_t *>(spare_scores));
    HIP_TRY(hipGetLastError());
    // (the sorted tuples, the flags and their sum are read no more: rank, is_new and new_pos take their buffers)
    return merge_into_store(b, p[3], spare_scores, nb, sorted, spare, p[2]);
}

// a checked chunk: its ghost nodes, halved for as long as a part does not fit the workspace
int add_checked(epik_amd_builder *b, const float *d_logp, const uint32_t *d_branch_of, uint64_t G)
{
    std::vector<std::pair<uint64_t, uint64_t>> todo{{0, G}};
    while (!todo.empty()) {
        const auto [g0, g1] = todo.back();
        todo.pop_back();
        bool too_large = false;
        uint64_t need = 0;
        if (const int rc = add_range(b, d_logp, d_branch_of, g0, g1, &too_large, &need); rc != EPIK_AMD_OK) return rc;
        if (!too_large) continue;
        if (g1 - g0 == 1)
            return fail_with(EPIK_AMD_ERR_INVALID, "ghost node " + std::to_string(g0) + " of the chunk needs a workspace of " + std::to_string(need) +
                                                       " bytes, the builder has " + std::to_string(b->ws_bytes) +
                                                       " (the ghost nodes before it were added; the others were not)");
        ++b->splits;
        const uint64_t mid = g0 + (g1 - g0) / 2;
        todo.push_back({mid, g1});
        todo.push_back({g0, mid});
    }
    return EPIK_AMD_OK;
}

int check_builder(const epik_amd_builder *b)
{
    if (!b) return fail_with(EPIK_AMD_ERR_INVALID, "null builder");
    if (b->device < 0) return fail_with(EPIK_AMD_ERR_INVALID, "the result of epik_amd_build_host takes no more chunks");
    return EPIK_AMD_OK;
}

int add_impl(epik_amd_builder *b, const float *logp, const uint32_t *branch_of, uint64_t G, uint64_t L, bool on_device)
{
    if (const int rc = check_builder(b); rc != EPIK_AMD_OK) return rc;
    std::string err;
    if (const int rc = build_check_length(L, b->k, b->L, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
    if (G == 0) return EPIK_AMD_OK;
    if (!logp || !branch_of) return fail_with(EPIK_AMD_ERR_INVALID, on_device ? "null device buffer" : "null host buffer");
    HIP_TRY(hipSetDevice(b->device));
    const uint64_t n = G * L * b->sigma;
    struct Upload {  // (the host chunk on the device, freed however the call ends)
        void *logp = nullptr, *branch_of = nullptr;
        ~Upload()
        {
            if (logp) (void)hipFree(logp);
            if (branch_of) (void)hipFree(branch_of);
        }
    } up;
    const float *d_logp = logp;
    const uint32_t *d_branch_of = branch_of;
    if (!on_device) {
        if (const int rc = build_check_chunk(logp, branch_of, G, L, b->sigma, b->num_branches, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        HIP_TRY(hipMalloc(&up.logp, n * sizeof(float)));
        HIP_TRY(hipMalloc(&up.branch_of, G * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(up.logp, logp, n * sizeof(float), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(up.branch_of, branch_of, G * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
        d_logp = static_cast<const float *>(up.logp), d_branch_of = static_cast<const uint32_t *>(up.branch_of);
    } else {
        HIP_TRY(hipMemsetAsync(b->d_words, 0xff, 2 * sizeof(unsigned long long), b->stream));
        hipLaunchKernelGGL(validate_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, b->stream, d_logp, n, d_branch_of, G, b->num_branches,
                           b->d_words);
        HIP_TRY(hipGetLastError());
        unsigned long long words[2];
        HIP_TRY(hipMemcpyAsync(words, b->d_words, sizeof words, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        if (words[0] != ~0ull) {
            float value = 0;
            HIP_TRY(hipMemcpy(&value, d_logp + words[0], sizeof value, hipMemcpyDeviceToHost));
            return fail_with(EPIK_AMD_ERR_INVALID, build_bad_value(words[0], L, b->sigma, value));
        }
        if (words[1] != ~0ull) {
            uint32_t branch = 0;
            HIP_TRY(hipMemcpy(&branch, d_branch_of + words[1], sizeof branch, hipMemcpyDeviceToHost));
            return fail_with(EPIK_AMD_ERR_INVALID, build_bad_branch(words[1], branch, b->num_branches));
        }
    }
    b->L = L;
    b->finished = false;
    const int rc = add_checked(b, d_logp, d_branch_of, G);
    (void)hipStreamSynchronize(b->stream);
    return rc;
}

void free_finished(epik_amd_builder *b)
{
    if (b->d_keys) (void)hipFree(b->d_keys);
    if (b->d_offsets) (void)hipFree(b->d_offsets);
    if (b->d_values) (void)hipFree(b->d_values);
    b->d_keys = nullptr, b->d_offsets = nullptr, b->d_values = nullptr;
}

int finish_device(epik_amd_builder *b)
{
    HIP_TRY(hipSetDevice(b->device));
    free_finished(b);
    const uint64_t n = b->store_n;
    b->num_entries = n, b->num_keys = 0;
    if (n == 0) return EPIK_AMD_OK;
    struct Scratch {
        uint64_t *flags = nullptr, *pos = nullptr;
        ~Scratch()
        {
            if (flags) (void)hipFree(flags);
            if (pos) (void)hipFree(pos);
        }
    } sc;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc.flags), (n + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc.pos), (n + 1) * sizeof(uint64_t)));
    hipLaunchKernelGGL(head_flag_kernel, dim3(blocks_for(n + 1)), dim3(kBlock), 0, b->stream, b->store_packed, n, b->branch_bits, sc.flags);
    HIP_TRY(hipGetLastError());
    if (const int rc = exclusive_sum(b, sc.flags, sc.pos, n + 1); rc != EPIK_AMD_OK) return rc;
    if (const int rc = read_word(b, sc.pos + n, b->num_keys); rc != EPIK_AMD_OK) return rc;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b->d_keys), b->num_keys * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b->d_offsets), (b->num_keys + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b->d_values), n * sizeof(epik_amd_pkdb_value)));
    hipLaunchKernelGGL(csr_kernel, dim3(blocks_for(n + 1)), dim3(kBlock), 0, b->stream, b->store_packed, b->store_score, sc.pos, n,
                       b->branch_bits, b->num_keys, b->d_keys, b->d_offsets, b->d_values);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_builder_create(int device, uint32_t sigma, uint32_t k, uint32_t num_branches, float log_thr, uint64_t workspace_bytes,
                            epik_amd_builder **builder)
{
    if (!builder) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *builder = nullptr;
    std::string err;
    if (const int rc = build_check_params(sigma, k, num_branches, log_thr, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail_with(EPIK_AMD_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail_with(EPIK_AMD_ERR_INVALID, "device " + std::to_string(device) + " does not exist");
    try {
        auto *b = new epik_amd_builder;
        b->device = device, b->sigma = sigma, b->k = k, b->num_branches = num_branches, b->log_thr = log_thr;
        b->prune_thr = build_prune_threshold(log_thr, k);
        b->branch_bits = bits_for(num_branches);
        uint64_t codes = 1;
        for (uint32_t j = 0; j < k; ++j) codes *= sigma;
        b->key_bits = bits_for(codes);
        b->ws_bytes = workspace_bytes ? workspace_bytes : 1ull << 30;
        const auto fail = [&](hipError_t e, const char *what) {
            epik_amd_builder_destroy(b);
            return fail_with(EPIK_AMD_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        };
        if (const hipError_t e = hipSetDevice(device); e != hipSuccess) return fail(e, "hipSetDevice");
        if (const hipError_t e = hipStreamCreate(&b->stream); e != hipSuccess) return fail(e, "hipStreamCreate");
        if (const hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->ws), b->ws_bytes); e != hipSuccess) return fail(e, "hipMalloc of the workspace");
        if (const hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_words), 2 * sizeof(unsigned long long)); e != hipSuccess)
            return fail(e, "hipMalloc");
        *builder = b;
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("builder_create: ") + e.what());
    }
}

int epik_amd_builder_add(epik_amd_builder *builder, const float *logp, const uint32_t *branch_of, uint64_t G, uint64_t L)
{
    try {
        return add_impl(builder, logp, branch_of, G, L, false);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("builder_add: ") + e.what());
    }
}

int epik_amd_builder_add_device(epik_amd_builder *builder, const void *d_logp, const void *d_branch_of, uint64_t G, uint64_t L)
{
    try {
        return add_impl(builder, static_cast<const float *>(d_logp), static_cast<const uint32_t *>(d_branch_of), G, L, true);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("builder_add_device: ") + e.what());
    }
}

int epik_amd_builder_finish(epik_amd_builder *builder, uint64_t *num_keys, uint64_t *num_entries, uint64_t *num_splits)
{
    if (!builder || !num_keys || !num_entries) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    if (builder->device >= 0 && !builder->finished) {
        if (const int rc = finish_device(builder); rc != EPIK_AMD_OK) return rc;
        builder->finished = true;
    }
    *num_keys = builder->num_keys, *num_entries = builder->num_entries;
    if (num_splits) *num_splits = builder->splits;
    return EPIK_AMD_OK;
}

int epik_amd_builder_copy(epik_amd_builder *builder, uint32_t *keys, uint64_t *offsets, epik_amd_pkdb_value *values)
{
    if (!builder || !offsets) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    if (!builder->finished) return fail_with(EPIK_AMD_ERR_INVALID, "builder_copy before builder_finish");
    const uint64_t K = builder->num_keys, E = builder->num_entries;
    if ((K && !keys) || (E && !values)) return fail_with(EPIK_AMD_ERR_INVALID, "null host buffer");
    if (builder->device < 0) {
        if (K) std::memcpy(keys, builder->host.keys.data(), K * sizeof(uint32_t));
        std::memcpy(offsets, builder->host.offsets.data(), (K + 1) * sizeof(uint64_t));
        if (E) std::memcpy(values, builder->host.values.data(), E * sizeof(epik_amd_pkdb_value));
        return EPIK_AMD_OK;
    }
    offsets[0] = 0;
    if (E == 0) return EPIK_AMD_OK;
    HIP_TRY(hipSetDevice(builder->device));
    HIP_TRY(hipMemcpy(keys, builder->d_keys, K * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(offsets, builder->d_offsets, (K + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(values, builder->d_values, E * sizeof(epik_amd_pkdb_value), hipMemcpyDeviceToHost));
    return EPIK_AMD_OK;
}

int epik_amd_builder_rank(epik_amd_builder *builder, uint32_t filter, uint64_t seed, double *value, uint32_t *order)
{
    if (!builder) return fail_with(EPIK_AMD_ERR_INVALID, "null builder");
    if (!builder->finished) return fail_with(EPIK_AMD_ERR_INVALID, "builder_rank before builder_finish");
    const uint64_t K = builder->num_keys;
    if (K && (!value || !order)) return fail_with(EPIK_AMD_ERR_INVALID, "null host buffer");
    try {
        std::string err;
        if (builder->device < 0) {
            const int rc = filter_rank_host(builder->num_branches, builder->log_thr, builder->host.keys.data(), builder->host.offsets.data(),
                                            builder->host.values.data(), K, filter, seed, 1, value, order, err);
            return rc == EPIK_AMD_OK ? rc : fail_with(rc, err);
        }
        if (const int rc = filter_check_params(builder->num_branches, builder->log_thr, filter, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        if (K == 0) return EPIK_AMD_OK;
        HIP_TRY(hipSetDevice(builder->device));
        const uint64_t o_order = align_up(K * sizeof(double));  // value | order on the device, kept by the handle
        if (const int rc = filter_scratch_reserve(builder->rank_out, o_order + K * sizeof(uint32_t), builder->stream); rc != EPIK_AMD_OK) return rc;
        uint8_t *base = static_cast<uint8_t *>(builder->rank_out.base);
        if (const int rc = filter_rank_on_device(builder->device, builder->num_branches, builder->log_thr, builder->d_keys, builder->d_offsets,
                                                 builder->d_values, K, filter, seed, reinterpret_cast<double *>(base),
                                                 reinterpret_cast<uint32_t *>(base + o_order), builder->stream, &builder->rank_scratch);
            rc != EPIK_AMD_OK)
            return rc;
        HIP_TRY(hipMemcpy(value, base, K * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(order, base + o_order, K * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("builder_rank: ") + e.what());
    }
}

void epik_amd_builder_destroy(epik_amd_builder *builder)
{
    if (!builder) return;
    if (builder->device >= 0) {
        (void)hipSetDevice(builder->device);
        if (builder->stream) (void)hipStreamSynchronize(builder->stream);
        free_finished(builder);
        filter_scratch_free(builder->rank_scratch), filter_scratch_free(builder->rank_out);
        if (builder->store_packed) (void)hipFree(builder->store_packed);
        if (builder->store_score) (void)hipFree(builder->store_score);
        if (builder->ws) (void)hipFree(builder->ws);
        if (builder->temp) (void)hipFree(builder->temp);
        if (builder->d_words) (void)hipFree(builder->d_words);
        if (builder->stream) (void)hipStreamDestroy(builder->stream);
    }
    delete builder;
}

int epik_amd_build_host(uint32_t sigma, uint32_t k, uint32_t num_branches, float log_thr, const float *logp, const uint32_t *branch_of,
                        uint64_t G, uint64_t L, uint32_t num_threads, epik_amd_builder **result)
{
    if (!result) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *result = nullptr;
    try {
        std::string err;
        if (const int rc = build_check_params(sigma, k, num_branches, log_thr, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        if (const int rc = build_check_length(L, k, 0, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        if (G)
            if (const int rc = build_check_chunk(logp, branch_of, G, L, sigma, num_branches, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        auto b = std::make_unique<epik_amd_builder>();
        b->sigma = sigma, b->k = k, b->num_branches = num_branches, b->log_thr = log_thr, b->L = L;
        if (const int rc = build_rule_host(sigma, k, log_thr, logp, branch_of, G, L, num_threads, b->host, err); rc != EPIK_AMD_OK)
            return fail_with(rc, err);
        b->num_keys = b->host.keys.size(), b->num_entries = b->host.values.size();
        b->finished = true;
        *result = b.release();
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("build_host: ") + e.what());
    }
}

}  // extern "C"
