// permanova_place.hip -- PERMANOVA (Anderson 2001) of a cohort's samples over their KR distances on the device: are the
// groups of a factor column different?  epik_amd_cohort_permanova_device / _permanova / _permanova_host / _permanova_kr_host
// (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h beside the KR rule (DESIGN.md 3.15;
// epik_amd/host/cohort.cpp: permanova_records_of_kr is the same rule on the CPU).  Every sum is a sequential chain from +0.0
// in one lane (__dadd_rn / __dmul_rn / __ddiv_rn; the file is built with -ffp-contract=off as well); a rank is a count or the
// slot of a sort, exact either way; the count of the permutations at most SSW_0 is an integer sum.  NA is stored as its bit
// pattern and never computed.
//
//   permanova_square_kernel   A2 = KR * KR, the whole matrix once a call: no permutation multiplies again.
//   permanova_columns_kernel  a wave a column: U_c in list order and the groups by first appearance (ballots keep the
//                             order), the whole column's test and its record.
//   permanova_pairs_kernel    a wave a (column, pair slot): the sub-list of the two groups, its test and its record.
//                             Both append a defined test to the list of the tests to run.
//   permanova_ssw_kernel      a workgroup a (test, kPerms labellings): the labellings of kPerms permutations side by side
//                             as the four bytes of a word per position, so that one read of A2[j][i] serves four chains.
//                             Lane q owns the rows q and n - 1 - q (n - 1 steps together: the triangle is level) and reads
//                             A2[u_j][u_i] for a j that the wave shares: a coalesced line.  Then a lane a (labelling,
//                             group): W_g, and a lane a labelling: SSW.  The keys are ranked by counting up to
//                             kCountPositions positions and by a bitonic sort of (key, position) beyond; the labellings,
//                             keys and row sums of a test of up to kLdsPositions positions stay in LDS, beyond (or with
//                             EPIK_AMD_PERMANOVA_LDS=0) in the workgroup's slice of global memory, ranked by counting:
//                             the same code on other pointers.  Launched twice: the observed labelling beside the
//                             labelling with one group (whose W_0 is T) for SSW_0, ss_total, f, r2 and the groups' sums;
//                             then the permutations 1 .. P, each unit adding its count to at_most with a vector atomic.
//   permanova_finish_kernel   p = (1 + at_most) / (P + 1), and NA into the ssw of the tests that did not run.
//   permanova_strata_kernel   with strata only (the strata rule of include/epik_amd.h): the tables of every
//                             test's list, once a call; the permutations then run in permanova_ssw_kernel's kStrata
//                             instantiation, whose LDS tier ends at kLdsStrataPositions.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kColumns = EPIK_AMD_PERMANOVA_MAX_COLUMNS;
constexpr uint32_t kGroups = EPIK_AMD_PERMANOVA_MAX_GROUPS;
constexpr uint32_t kPairGroups = EPIK_AMD_PERMANOVA_MAX_PAIR_GROUPS;
constexpr uint32_t kPairSlots = EPIK_AMD_PERMANOVA_PAIR_SLOTS;
constexpr uint32_t kMissing = EPIK_AMD_PERMANOVA_MISSING;
constexpr uint32_t kPerms = 4;              // the labellings a workgroup carries through one pass over A2: the bytes of a word
constexpr uint32_t kLdsPositions = 1024;    // the most positions of a test whose vectors stay in LDS (62 KiB with the rest)
constexpr uint32_t kLdsStrataPositions = 512;  // ... with strata: their two tables beside the rest would make 70 KiB at 1 024
constexpr uint32_t kCountPositions = 256;   // up to here the LDS path ranks by counting; beyond, it sorts
constexpr uint32_t kSmallSamples = 128;     // up to here a workgroup is one wave
constexpr uint32_t kGeneralBlocks = 256;    // workgroups of the general path: each has a slice
constexpr uint64_t kManyBlocks = 65536;

static_assert(sizeof(epik_amd_permanova) == 56, "the record is 56 bytes");
static_assert(kPairSlots == kPairGroups * (kPairGroups - 1) / 2 && kPerms == 4 && kBlock == 256 && kWave == 64);
static_assert(kCountPositions <= kLdsPositions && (kLdsPositions & (kLdsPositions - 1)) == 0);

struct PermColumn {
    uint32_t used, groups;
    uint32_t size[kGroups];
};

struct PermTest {
    uint64_t offset;   // of its list in the pools
    uint32_t n, groups, column, defined;
    uint32_t size[2];  // of a pair's two groups (the whole column's are in its PermColumn)
    double ssw0;
};

struct PermSpace {
    double *A2;         // [S][S]
    double *scratch;    // [kGeneralBlocks] x (t[kPerms][Sp] | keys[Sp] | mu[Sp])
    uint32_t *lab;      // [M][Sp]: the labels by sample
    uint32_t *idx;      // [M][lists * Sp]: the samples of a test's positions; a column's pairs follow its whole list
    uint32_t *active;   // [tests], then the counter
    PermColumn *cols;   // [M]
    PermTest *tests;    // [M][1 + Q]
    uint8_t *lam;       // as idx: the groups of the positions
    uint32_t *strata;   // with strata only: [Sp], the strata by sample
    uint32_t *hs, *home;  // ... and as idx: the strata of a test's positions, and its positions by (stratum, position)
};

constexpr size_t kSliceBytes = kPerms * 8 + 8 + 4;  // the bytes of a slice per padded sample

size_t permanova_space(void *base, uint32_t S, uint32_t padded, uint32_t M, bool pairwise, bool strata, PermSpace *sp)
{
    const size_t slots = 1 + (pairwise ? kPairSlots : 0), lists = pairwise ? kPairGroups : 1, tests = M * slots;
    Carver c(base);
    const PermSpace parts{.A2 = c.take<double>((size_t)S * S),
                          .scratch = c.take<double>((size_t)kGeneralBlocks * kSliceBytes * padded / sizeof(double)),
                          .lab = c.take<uint32_t>((size_t)M * padded),
                          .idx = c.take<uint32_t>((size_t)M * lists * padded),
                          .active = c.take<uint32_t>(tests + 1),
                          .cols = c.take<PermColumn>(M),
                          .tests = c.take<PermTest>(tests),
                          .lam = c.take<uint8_t>((size_t)M * lists * padded),
                          .strata = c.take<uint32_t>(strata ? padded : 0),
                          .hs = c.take<uint32_t>(strata ? (size_t)M * lists * padded : 0),
                          .home = c.take<uint32_t>(strata ? (size_t)M * lists * padded : 0)};
    if (sp) *sp = parts;
    return c.bytes();
}

__device__ inline void na_record(epik_amd_permanova *r, uint32_t used, uint32_t groups)
{
    r->used = used, r->groups = groups, r->at_most = 0;
    r->ss_total = r->ss_within = r->f = r->r2 = r->p = na_value();
}

__global__ __launch_bounds__(kBlock) void permanova_square_kernel(const double *__restrict__ kr, uint64_t cells, double *__restrict__ A2)
{
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const double d = kr[e];
        A2[e] = __dmul_rn(d, d);
    }
}

__global__ __launch_bounds__(kWave) void permanova_columns_kernel(const uint64_t *__restrict__ total, const uint32_t *__restrict__ lab,
                                                                  uint32_t num_samples, uint32_t padded, uint32_t num_columns,
                                                                  uint32_t slots, uint32_t lists, uint32_t *__restrict__ idx,
                                                                  uint8_t *__restrict__ lam, PermColumn *__restrict__ cols,
                                                                  PermTest *__restrict__ tests, uint32_t *__restrict__ active,
                                                                  epik_amd_permanova *__restrict__ out, double *__restrict__ group_ss)
{
    __shared__ uint32_t group_of[kGroups], size[kGroups];
    for (uint32_t c = blockIdx.x; c < num_columns; c += gridDim.x) {
        if (group_ss)
            for (uint32_t g = threadIdx.x; g < kGroups; g += kWave) group_ss[(uint64_t)c * kGroups + g] = na_value();
        const uint64_t offset = (uint64_t)c * lists * padded;
        uint32_t L, G;  // (uniform)
        column_list<kGroups>(total, lab + (uint64_t)c * padded, num_samples, kMissing, group_of, size, idx + offset, lam + offset, L, G);
        for (uint32_t g = threadIdx.x; g < kGroups; g += kWave) cols[c].size[g] = size[g];
        if (threadIdx.x == 0) {
            const bool defined = G >= 2 && L >= G + 1;
            cols[c].used = L, cols[c].groups = G;
            PermTest &t = tests[(uint64_t)c * slots];
            t.offset = offset, t.n = L, t.groups = G, t.column = c, t.defined = defined, t.size[0] = t.size[1] = 0, t.ssw0 = 0.0;
            na_record(out + (uint64_t)c * slots, L, G);
            if (defined) active[atomicAdd(active + (uint64_t)num_columns * slots, 1u)] = c * slots;
        }
        __syncthreads();  // (the tables are written again)
    }
}

__global__ __launch_bounds__(kWave) void permanova_pairs_kernel(uint32_t padded, uint32_t num_columns, uint32_t *__restrict__ idx,
                                                                uint8_t *__restrict__ lam, const PermColumn *__restrict__ cols,
                                                                PermTest *__restrict__ tests, uint32_t *__restrict__ active,
                                                                epik_amd_permanova *__restrict__ out)
{
    constexpr uint32_t slots = 1 + kPairSlots;
    for (uint32_t unit = blockIdx.x; unit < num_columns * kPairSlots; unit += gridDim.x) {
        const uint32_t c = unit / kPairSlots, pair = unit % kPairSlots;
        uint32_t h = 1;
        while ((h + 1) * h / 2 <= pair) ++h;
        const uint32_t g = pair - h * (h - 1) / 2, test = c * slots + 1 + pair;
        const uint32_t L = cols[c].used, G = cols[c].groups;
        if (h >= G) {
            if (threadIdx.x == 0) {
                PermTest &t = tests[test];
                t.offset = 0, t.n = 0, t.groups = 0, t.column = c, t.defined = 0, t.size[0] = t.size[1] = 0, t.ssw0 = 0.0;
                na_record(out + test, 0, 0);
            }
            continue;
        }
        // the pairs' lists follow the whole column's, in slot order
        const uint64_t column_at = (uint64_t)c * kPairGroups * padded;
        uint64_t offset = column_at + padded;
        for (uint32_t hh = 1; hh <= h; ++hh)
            for (uint32_t gg = 0; gg < (hh < h ? hh : g); ++gg) offset += cols[c].size[gg] + cols[c].size[hh];
        uint32_t n = 0;
        for (uint32_t base = 0; base < L; base += kWave) {
            const uint32_t i = base + threadIdx.x;
            const uint32_t group = i < L ? lam[column_at + i] : kMissing;
            n += append_in_order(group == g || group == h, n, i < L ? idx[column_at + i] : 0, group == h, idx + offset, lam + offset);
        }
        if (threadIdx.x == 0) {
            const bool defined = n >= 3;
            PermTest &t = tests[test];
            t.offset = offset, t.n = n, t.groups = 2, t.column = c, t.defined = defined;
            t.size[0] = cols[c].size[g], t.size[1] = cols[c].size[h], t.ssw0 = 0.0;
            na_record(out + test, n, 2);
            if (defined) active[atomicAdd(active + (uint64_t)num_columns * slots, 1u)] = test;
        }
    }
}

struct SswArgs {
    const double *A2;
    const uint32_t *idx;
    const uint8_t *lam;
    const PermColumn *cols;
    PermTest *tests;
    const uint32_t *active;  // the counter follows the `num_tests` entries
    double *scratch;
    epik_amd_permanova *out;
    double *ssw, *group_ss;  // or null
    uint64_t seed;
    uint32_t num_samples, padded, num_tests, slots, num_permutations, pitch;
    const uint32_t *hs, *home;  // the strata rule's tables, as idx; or null
};

// the strata rule's tables of every test with a list: a workgroup a test
__global__ __launch_bounds__(kBlock) void permanova_strata_kernel(const uint32_t *__restrict__ strata, const uint32_t *__restrict__ idx,
                                                                  const PermTest *__restrict__ tests, uint32_t num_tests, uint32_t *hs,
                                                                  uint32_t *home)
{
    for (uint32_t test = blockIdx.x; test < num_tests; test += gridDim.x) {  // (uniform)
        const uint32_t *list = idx + tests[test].offset;
        strata_tables(strata, [&](uint32_t i) { return list[i]; }, tests[test].n, hs + tests[test].offset, home + tests[test].offset);
    }
}

// the row sums of the kPerms labellings for row i: t[k] = the chain over j > i, ascending, with the same byte k
__device__ inline void row_sums(const double *__restrict__ A2, uint64_t S, const uint32_t *idx, const uint32_t *mu, uint32_t n,
                                uint32_t i, double *t, uint32_t pitch)
{
    const uint32_t mine = mu[i];
    const double *column = A2 + idx[i];
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll 4  // (the reads of four values are in flight ahead of the dependent adds)
    for (uint32_t j = i + 1; j < n; ++j) {
        const uint32_t differ = mu[j] ^ mine;
        const double a = column[(uint64_t)idx[j] * S];
        if (!(differ & 0x000000ffu)) t0 = __dadd_rn(t0, a);
        if (!(differ & 0x0000ff00u)) t1 = __dadd_rn(t1, a);
        if (!(differ & 0x00ff0000u)) t2 = __dadd_rn(t2, a);
        if (!(differ & 0xff000000u)) t3 = __dadd_rn(t3, a);
    }
    t[i] = t0, t[pitch + i] = t1, t[2 * pitch + i] = t2, t[3 * pitch + i] = t3;
}

// kObserved: the labellings lambda and "one group" of every test to run; else its permutations 1 .. P, kPerms a unit.
// kStrata: the arrangements of the strata rule: the ranking is by (stratum, key, position), and the slot's entry of home[] is
// the position whose label is taken.
template <bool kLds, bool kObserved, bool kStrata>
__global__ __launch_bounds__(kBlock) void permanova_ssw_kernel(const SswArgs a)
{
    extern __shared__ __align__(16) unsigned char dynamic_lds[];
    __shared__ double term[kPerms * kGroups];  // W_g / n_g of labelling k: term[k * G + g]
    __shared__ uint32_t size[kGroups];
    __shared__ double ssw_of[kPerms];
    const uint32_t tid = threadIdx.x, threads = blockDim.x, pitch = a.pitch;
    double *t;
    uint64_t *keys;
    uint32_t *mu, *pos = nullptr, *lds_idx = nullptr;
    uint8_t *lds_lam = nullptr;
    if (kLds) {
        t = reinterpret_cast<double *>(dynamic_lds);
        keys = reinterpret_cast<uint64_t *>(t + kPerms * pitch);
        mu = reinterpret_cast<uint32_t *>(keys + pitch);
        pos = mu + pitch, lds_idx = pos + pitch;
        lds_lam = reinterpret_cast<uint8_t *>(lds_idx + pitch);
    } else {
        // (kSliceBytes * pitch bytes a slice, pitch % 32 == 0: every slice is aligned)
        t = reinterpret_cast<double *>(reinterpret_cast<char *>(a.scratch) + (uint64_t)blockIdx.x * kSliceBytes * pitch);
        keys = reinterpret_cast<uint64_t *>(t + kPerms * pitch);
        mu = reinterpret_cast<uint32_t *>(keys + pitch);
    }
    uint8_t *mu8 = reinterpret_cast<uint8_t *>(mu);
    const uint32_t P = a.num_permutations, chunks = kObserved ? 1 : (P + kPerms - 1) / kPerms;
    const uint64_t units = (uint64_t)a.active[a.num_tests] * chunks, S = a.num_samples;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t test = a.active[unit / chunks], chunk = (uint32_t)(unit % chunks);
        const PermTest info = a.tests[test];
        const uint32_t n = info.n, G = info.groups;
        const bool whole = test % a.slots == 0;
        const uint32_t *idx = a.idx + info.offset;
        const uint8_t *lam = a.lam + info.offset;
        const uint32_t *hs = nullptr, *home = nullptr;
        if constexpr (kStrata) hs = a.hs + info.offset, home = a.home + info.offset;
        if (kLds) {
            for (uint32_t i = tid; i < n; i += threads) lds_idx[i] = idx[i], lds_lam[i] = lam[i];
            idx = lds_idx, lam = lds_lam;
            if constexpr (kStrata) {  // (the two tables follow the groups: pitch % 64 == 0)
                uint32_t *lds_hs = reinterpret_cast<uint32_t *>(lds_lam + pitch), *lds_home = lds_hs + pitch;
                for (uint32_t i = tid; i < n; i += threads) lds_hs[i] = hs[i], lds_home[i] = home[i];
                hs = lds_hs, home = lds_home;
            }
        }
        for (uint32_t g = tid; g < G; g += threads) size[g] = whole ? a.cols[info.column].size[g] : g ? info.size[1] : info.size[0];
        __syncthreads();
        const uint32_t p0 = kObserved ? 0 : 1 + chunk * kPerms, np = kObserved ? 2 : min(kPerms, P + 1 - p0);
        for (uint32_t k = 0; k < kPerms; ++k) {
            if (kObserved || k >= np) {  // lambda; beside it, when observed, the labelling with one group; else filling
                for (uint32_t i = tid; i < n; i += threads) mu8[i * kPerms + k] = kObserved && k > 0 ? 0 : lam[i];
                continue;
            }
            const uint32_t p = p0 + k;
            for (uint32_t i = tid; i < n; i += threads) keys[i] = permutation_key(a.seed, p, i);
            __syncthreads();
            if (kLds && n > kCountPositions) {
                // (key, position) sorted by a bitonic network over the next power of two, the padding above every pair:
                // the slot of a pair is its rank
                uint32_t P2 = 2 * kCountPositions;
                while (P2 < n) P2 <<= 1;  // (<= pitch)
                for (uint32_t i = tid; i < P2; i += threads) {
                    pos[i] = i < n ? i : 0xffffffffu;
                    if (i >= n) keys[i] = ~0ull;
                }
                __syncthreads();
                for (uint32_t width = 2; width <= P2; width <<= 1)
                    for (uint32_t step = width >> 1; step > 0; step >>= 1) {
                        for (uint32_t e = tid; e < P2 / 2; e += threads) {
                            const uint32_t lo = 2 * e - (e & (step - 1)), hi = lo + step;  // (hi < P2)
                            const bool up = (lo & width) == 0;
                            const uint64_t ka = keys[lo], kc = keys[hi];
                            const uint32_t pa = pos[lo], pc = pos[hi];
                            bool above;
                            if constexpr (kStrata)  // (the padding's position is no index: its stratum is above every other)
                                above = strata_before(pc < n ? hs[pc] : 0xffffffffu, kc, pc, pa < n ? hs[pa] : 0xffffffffu, ka, pa);
                            else
                                above = ka > kc || (ka == kc && pa > pc);
                            if (above == up) keys[lo] = kc, keys[hi] = ka, pos[lo] = pc, pos[hi] = pa;
                        }
                        __syncthreads();
                    }
                for (uint32_t r = tid; r < n; r += threads) mu8[pos[r] * kPerms + k] = lam[kStrata ? home[r] : r];
            } else {
                for (uint32_t i = tid; i < n; i += threads) {
                    const uint64_t mine = keys[i];
                    uint32_t rank = 0;
#pragma unroll 4
                    for (uint32_t j = 0; j < n; ++j) {
                        const uint64_t other = keys[j];  // a broadcast
                        if constexpr (kStrata) rank += strata_before(hs[j], other, j, hs[i], mine, i);
                        else rank += other < mine || (other == mine && j < i);
                    }
                    mu8[i * kPerms + k] = lam[kStrata ? home[rank] : rank];
                }
            }
            __syncthreads();  // (the keys are written again)
        }
        __syncthreads();
        // the rows q and n - 1 - q in one lane: n - 1 steps whatever q
        for (uint32_t q = tid; q < (n + 1) / 2; q += threads) {
            row_sums(a.A2, S, idx, mu, n, q, t, pitch);
            if (n - 1 - q != q) row_sums(a.A2, S, idx, mu, n, n - 1 - q, t, pitch);
        }
        __syncthreads();
        for (uint32_t e = tid; e < kPerms * G; e += threads) {
            const uint32_t k = e / G, g = e % G;
            const double *tk = t + k * pitch;
            double w = 0.0;
#pragma unroll 4
            for (uint32_t i = 0; i < n; ++i)
                if (mu8[i * kPerms + k] == g) w = __dadd_rn(w, tk[i]);
            term[e] = kObserved && k > 0 ? w : __ddiv_rn(w, (double)size[g]);  // (observed, k = 1, g = 0: T itself)
        }
        __syncthreads();
        if (tid < kPerms) {
            double acc = 0.0;
            for (uint32_t g = 0; g < G; ++g) acc = __dadd_rn(acc, term[tid * G + g]);
            ssw_of[tid] = acc;
        }
        __syncthreads();
        if (kObserved) {
            if (whole && a.group_ss)
                for (uint32_t g = tid; g < G; g += threads) a.group_ss[(uint64_t)info.column * kGroups + g] = term[g];
            if (tid == 0) {
                const double ssw0 = ssw_of[0], total = __ddiv_rn(term[G], (double)n), among = __dsub_rn(total, ssw0);
                epik_amd_permanova *r = a.out + test;
                r->ss_total = total, r->ss_within = ssw0;  // (f, r2: NA from the tests' kernels)
                if (total != 0.0) {
                    r->r2 = __ddiv_rn(among, total);
                    if (ssw0 != 0.0) r->f = __ddiv_rn(__ddiv_rn(among, (double)(G - 1)), __ddiv_rn(ssw0, (double)(n - G)));
                }
                a.tests[test].ssw0 = ssw0;
                if (a.ssw) a.ssw[(uint64_t)test * (P + 1)] = ssw0;
            }
        } else if (tid == 0) {
            unsigned long long count = 0;
            for (uint32_t k = 0; k < np; ++k) {
                const double v = ssw_of[k];
                if (a.ssw) a.ssw[(uint64_t)test * (P + 1) + p0 + k] = v;
                count += v <= info.ssw0;
            }
            if (count) atomicAdd(reinterpret_cast<unsigned long long *>(&a.out[test].at_most), count);
        }
        __syncthreads();  // (the vectors and the sums are written again)
    }
}

__global__ __launch_bounds__(kBlock) void permanova_finish_kernel(const PermTest *__restrict__ tests, uint32_t num_tests,
                                                                  uint32_t num_permutations, epik_amd_permanova *__restrict__ out,
                                                                  double *__restrict__ ssw)
{
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t test = first; test < num_tests; test += stride)
        if (tests[test].defined)
            out[test].p = __ddiv_rn((double)(1 + out[test].at_most), (double)(num_permutations + 1));
    if (!ssw) return;
    const uint64_t row = (uint64_t)num_permutations + 1;
    for (uint64_t e = first; e < num_tests * row; e += stride)
        if (!tests[e / row].defined) ssw[e] = na_value();
}

int check_arguments(const uint32_t *labels, uint32_t S, uint32_t M, uint32_t P, bool pairwise)
{
    std::string err;
    return rule_result(permanova_arguments_valid(labels, S, M, P, pairwise, err), err);
}

int permanova_device_impl(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, const uint32_t *strata, uint32_t M,
                          uint32_t P, uint64_t seed, bool pairwise, void *d_out, void *d_ssw, void *d_group_ss, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_columns(M));
    COHORT_TRY(check_present(d_kr, labels, d_out));
    const uint32_t S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    COHORT_TRY(check_arguments(labels, S, M, P, pairwise));
    COHORT_TRY(check_has_distances(cohort));
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());  // (the distances enqueued on whatever stream, and an earlier call that reads the workspace)
    COHORT_TRY(cohort_space_ensure(cohort, kSpacePermanova, permanova_space(nullptr, S, padded, M, pairwise, strata != nullptr, nullptr)));
    PermSpace sp;
    permanova_space(cohort->space[kSpacePermanova].d, S, padded, M, pairwise, strata != nullptr, &sp);
    COHORT_TRY(upload_labels_by_column(labels, S, M, padded, kMissing, sp.lab));
    if (strata) COHORT_TRY(upload_strata(strata, S, padded, sp.strata));
    const uint32_t slots = 1 + (pairwise ? kPairSlots : 0), lists = pairwise ? kPairGroups : 1, tests = M * slots;
    HIP_TRY(hipMemsetAsync(sp.active + tests, 0, sizeof(uint32_t), stream));
    auto *out = static_cast<epik_amd_permanova *>(d_out);
    const uint64_t cells = (uint64_t)S * S;
    hipLaunchKernelGGL(permanova_square_kernel, cohort_grid(cohort, (cells + kBlock - 1) / kBlock, kManyBlocks), dim3(kBlock), 0, stream,
                       static_cast<const double *>(d_kr), cells, sp.A2);
    hipLaunchKernelGGL(permanova_columns_kernel, cohort_grid(cohort, M, kColumns), dim3(kWave), 0, stream, cohort->d_total, sp.lab, S, padded,
                       M, slots, lists, sp.idx, sp.lam, sp.cols, sp.tests, sp.active, out, static_cast<double *>(d_group_ss));
    if (pairwise)
        hipLaunchKernelGGL(permanova_pairs_kernel, cohort_grid(cohort, (uint64_t)M * kPairSlots, kManyBlocks), dim3(kWave), 0, stream, padded,
                           M, sp.idx, sp.lam, sp.cols, sp.tests, sp.active, out);
    if (strata)
        hipLaunchKernelGGL(permanova_strata_kernel, cohort_grid(cohort, tests, kManyBlocks), dim3(kBlock), 0, stream, sp.strata, sp.idx,
                           sp.tests, tests, sp.hs, sp.home);
    // (=0, tests: the general path whatever S)
    const bool lds = lds_switch("EPIK_AMD_PERMANOVA_LDS", S, strata ? kLdsStrataPositions : kLdsPositions);
    uint32_t pitch = padded;  // the general path's; the LDS path's: a power of two, for the sort
    if (lds)
        for (pitch = kWave; pitch < S; pitch <<= 1) {}
    const SswArgs args{sp.A2, sp.idx, sp.lam, sp.cols, sp.tests, sp.active, sp.scratch, out, static_cast<double *>(d_ssw),
                       static_cast<double *>(d_group_ss), seed, S, padded, tests, slots, P, pitch, strata ? sp.hs : nullptr,
                       strata ? sp.home : nullptr};
    const size_t dynamic = lds ? (size_t)pitch * (kPerms * 8 + 8 + 4 + 4 + 4 + 1 + (strata ? 4 + 4 : 0)) : 0;
    const dim3 block(S <= kSmallSamples ? kWave : kBlock);
    const uint64_t chunks = (P + kPerms - 1) / kPerms, most = lds ? kManyBlocks : kGeneralBlocks;
    const dim3 observed = cohort_grid(cohort, tests, most), permuted = cohort_grid(cohort, tests * chunks, most);
    if (lds) {
        hipLaunchKernelGGL((permanova_ssw_kernel<true, true, false>), observed, block, dynamic, stream, args);
        if (strata) hipLaunchKernelGGL((permanova_ssw_kernel<true, false, true>), permuted, block, dynamic, stream, args);
        else hipLaunchKernelGGL((permanova_ssw_kernel<true, false, false>), permuted, block, dynamic, stream, args);
    } else {
        hipLaunchKernelGGL((permanova_ssw_kernel<false, true, false>), observed, block, 0, stream, args);
        if (strata) hipLaunchKernelGGL((permanova_ssw_kernel<false, false, true>), permuted, block, 0, stream, args);
        else hipLaunchKernelGGL((permanova_ssw_kernel<false, false, false>), permuted, block, 0, stream, args);
    }
    const uint64_t finish = d_ssw ? (uint64_t)tests * (P + 1) : tests;
    hipLaunchKernelGGL(permanova_finish_kernel, cohort_grid(cohort, (finish + kBlock - 1) / kBlock, kManyBlocks), dim3(kBlock), 0, stream,
                       sp.tests, tests, P, out, static_cast<double *>(d_ssw));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_permanova_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, uint32_t num_columns,
                                     uint32_t num_permutations, uint64_t seed, int pairwise, void *d_out, void *d_ssw,
                                     void *d_group_ss, void *stream)
{
    return epik_amd_cohort_permanova_strata_device(cohort, d_kr, labels, num_columns, num_permutations, seed, pairwise, d_out, d_ssw,
                                                   d_group_ss, stream, nullptr);
}

int epik_amd_cohort_permanova_strata_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, uint32_t num_columns,
                                            uint32_t num_permutations, uint64_t seed, int pairwise, void *d_out, void *d_ssw,
                                            void *d_group_ss, void *stream, const uint32_t *strata)
{
    return guarded("cohort_permanova_device", [&]() -> int {
        return permanova_device_impl(cohort, d_kr, labels, strata, num_columns, num_permutations, seed, pairwise != 0, d_out, d_ssw,
                                     d_group_ss, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_permanova(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, const uint32_t *labels,
                              uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permanova *out,
                              double *ssw, double *group_ss)
{
    return epik_amd_cohort_permanova_metric(cohort, tree, branch_length, EPIK_AMD_DISTANCE_KR, labels, num_columns, num_permutations, seed,
                                            pairwise, out, ssw, group_ss);
}

int epik_amd_cohort_permanova_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                     const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                     epik_amd_permanova *out, double *ssw, double *group_ss)
{
    return epik_amd_cohort_permanova_strata(cohort, tree, branch_length, metric, labels, num_columns, num_permutations, seed, pairwise, out,
                                            ssw, group_ss, nullptr);
}

int epik_amd_cohort_permanova_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                     const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                     epik_amd_permanova *out, double *ssw, double *group_ss, const uint32_t *strata)
{
    return guarded("cohort_permanova", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_columns(num_columns));
        COHORT_TRY(check_present(labels, out));
        const uint32_t S = cohort->num_samples;
        COHORT_TRY(check_arguments(labels, S, num_columns, num_permutations, pairwise != 0));
        const size_t tests = (size_t)num_columns * (1 + (pairwise ? kPairSlots : 0));
        const size_t out_bytes = tests * sizeof(epik_amd_permanova), ssw_bytes = tests * ((size_t)num_permutations + 1) * sizeof(double);
        const size_t group_bytes = (size_t)num_columns * kGroups * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult kr, r, s, g;
        COHORT_TRY(kr.alloc((size_t)S * S * sizeof(double)));
        COHORT_TRY(r.alloc(out_bytes));
        COHORT_TRY(s.alloc(ssw_bytes, ssw != nullptr));
        COHORT_TRY(g.alloc(group_bytes, group_ss != nullptr));
        COHORT_TRY(cohort_distance_enqueue(cohort, tree, branch_length, metric, kr.d, nullptr));
        COHORT_TRY(permanova_device_impl(cohort, kr.d, labels, strata, num_columns, num_permutations, seed, pairwise != 0, r.d, s.d, g.d,
                                         nullptr));
        COHORT_TRY(r.copy_to(out, out_bytes));
        COHORT_TRY(s.copy_to(ssw, ssw_bytes));
        return g.copy_to(group_ss, group_bytes);
    });
}

int epik_amd_cohort_permanova_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                   const double *branch_length, const uint32_t *labels, uint32_t num_columns,
                                   uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permanova *out, double *ssw,
                                   double *group_ss)
{
    return epik_amd_cohort_permanova_metric_host(mass, num_samples, num_branches, first, branch_length, EPIK_AMD_DISTANCE_KR, labels,
                                                 num_columns, num_permutations, seed, pairwise, out, ssw, group_ss);
}

int epik_amd_cohort_permanova_metric_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                          const double *branch_length, uint32_t metric, const uint32_t *labels, uint32_t num_columns,
                                          uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permanova *out, double *ssw,
                                          double *group_ss)
{
    return epik_amd_cohort_permanova_strata_host(mass, num_samples, num_branches, first, branch_length, metric, labels, num_columns,
                                                 num_permutations, seed, pairwise, out, ssw, group_ss, nullptr);
}

int epik_amd_cohort_permanova_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                          const double *branch_length, uint32_t metric, const uint32_t *labels, uint32_t num_columns,
                                          uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permanova *out, double *ssw,
                                          double *group_ss, const uint32_t *strata)
{
    return guarded("cohort_permanova_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, labels, out));
        std::string err;
        return rule_result(permanova_records(mass, num_samples, num_branches, first, branch_length, labels, num_columns, num_permutations,
                                             seed, pairwise != 0, out, ssw, group_ss, err, metric, strata),
                           err);
    });
}

int epik_amd_cohort_permanova_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                      uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                      epik_amd_permanova *out, double *ssw, double *group_ss)
{
    return epik_amd_cohort_permanova_strata_kr_host(kr, totals, num_samples, labels, num_columns, num_permutations, seed, pairwise, out, ssw,
                                                    group_ss, nullptr);
}

int epik_amd_cohort_permanova_strata_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                             uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                             epik_amd_permanova *out, double *ssw, double *group_ss, const uint32_t *strata)
{
    return guarded("cohort_permanova_kr_host", [&]() -> int {
        COHORT_TRY(check_host_samples(num_samples));
        COHORT_TRY(check_present(kr, totals, labels, out));
        std::string err;
        return rule_result(permanova_records_of_kr(kr, totals, num_samples, labels, num_columns, num_permutations, seed, pairwise != 0, out,
                                                   ssw, group_ss, err, strata),
                           err);
    });
}

}  // extern "C"
