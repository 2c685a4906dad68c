// ancestral_place.hip -- ancestral posteriors of a reference tree's ghost nodes: epik_amd_ancestral_create,
// _posteriors, _posteriors_device, _destroy, epik_amd_ancestral_host, epik_amd_model_pmatrices and
// epik_amd_model_gamma_rates (include/epik_amd.h, where the rule is stated once).
//
// The reference project has no ancestral reconstruction; nothing of it is restated here.
//
// A chunk of sites goes through
//   down_kernel    level by level from the leaves: all inner nodes of one height in a launch, D_v = F(l) F(r), scaled;
//   up_kernel      level by level from the root: all nodes of one depth in a launch, U_v = F(sibling) G(parent), scaled;
//   ghost_kernel   one launch over all branches: the midpoint and the pendant node of every branch, float32.
// The grid of the two passes is (node of the level) x (tile of kTile sites); a workgroup has kTile x C threads and a
// thread owns one (site, category) with all its states in registers.  The two matrices of a node, C of each, are staged
// in LDS with the category stride padded by two doubles, so that lanes of different categories read different banks
// (nucleotides: a wave holds 64 / C sites of every category); for amino acids a wave holds one category of 64 sites and
// every LDS read is a broadcast.  The maximum of a site over its categories goes through LDS as well.
// ghost_kernel gives a site to a thread, which walks the categories in order -- the sum over categories is ordered by
// the rule -- and reads the matrices with uniform (scalar) loads.
// Leaves are never stored as doubles: a child that is a leaf is read from its mask.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../host/ancestral.hpp"
#include "host_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kTile = EPIK_AMD_ANCESTRAL_TILE_SITES;
constexpr uint32_t kLeafFlag = 0x80000000u;  // a source that is a row of the masks, not a slot of the partials
constexpr uint64_t kMaxTiles = 65535;        // gridDim.y
static_assert(kTile == kWave, "a wave is a tile of sites of one category (amino acids)");

// One node of a level: out = F(a) * F(b), or F(a) alone (b_mat = kAncestralNone)
struct Job {
    uint32_t out_slot;
    uint32_t a_mat, a_src;  // the node whose branch gives the matrix; where its vector is
    uint32_t b_mat, b_src;
};

}  // namespace

struct epik_amd_ancestral {
    int device = -1;
    uint32_t N = 0, S = 0, C = 0, n_inner = 0, n_leaves = 0;
    uint64_t ws_bytes = 0, site_bytes = 0, chunk_sites = 0;
    hipStream_t stream = nullptr;
    uint8_t *ws = nullptr;
    double *d_tables = nullptr;  // p_full | p_half | p_pend | weights | pi
    Job *d_jobs = nullptr;       // the down levels, then the up levels
    uint32_t *d_ghost_src = nullptr;  // per branch where D_b is
    unsigned long long *d_dead = nullptr;
    std::vector<std::pair<uint64_t, uint32_t>> down_levels, up_levels;  // (first job, jobs)
};

namespace {

template <uint32_t S>
__device__ inline void load_vector(const double *__restrict__ part, const uint32_t *__restrict__ masks, uint32_t src, uint64_t Lc,
                                   uint32_t C, uint64_t site, uint32_t c, double (&v)[S])
{
    if (src & kLeafFlag) {
        constexpr uint32_t full = (1u << S) - 1;
        uint32_t m = masks[(uint64_t)(src & ~kLeafFlag) * Lc + site] & full;
        if (m == 0) m = full;
#pragma unroll
        for (uint32_t y = 0; y < S; ++y) v[y] = (m >> y & 1u) ? 1.0 : 0.0;
    } else {
        const double2 *p = reinterpret_cast<const double2 *>(part + (((uint64_t)src * Lc + site) * C + c) * S);
#pragma unroll
        for (uint32_t y = 0; y < S / 2; ++y) {
            const double2 d = p[y];
            v[2 * y] = d.x, v[2 * y + 1] = d.y;
        }
    }
}

// f[x] = sum over y of P[x][y] * v[y], from the first term
template <uint32_t S>
__device__ inline void mat_vec(const double *P, const double (&v)[S], double (&f)[S])
{
#pragma unroll
    for (uint32_t x = 0; x < S; ++x) {
        double acc = P[x * S] * v[0];
#pragma unroll
        for (uint32_t y = 1; y < S; ++y) acc = acc + P[x * S + y] * v[y];
        f[x] = acc;
    }
}

// LDS of a pass: two sets of C matrices and the maxima of kTile x C threads
template <uint32_t S>
constexpr uint32_t mat_stride() { return S * S + 2; }
template <uint32_t S>
size_t pass_lds_bytes(uint32_t C) { return ((size_t)2 * C * mat_stride<S>() + (size_t)kTile * C) * sizeof(double); }

template <uint32_t S>
__device__ inline void combine_tile(const Job job, double *__restrict__ part, const uint32_t *__restrict__ masks,
                                    const double *__restrict__ p_full, uint64_t Lc, uint32_t C)
{
    extern __shared__ double lds[];
    constexpr uint32_t kStride = mat_stride<S>();
    double *Pa = lds, *Pb = Pa + C * kStride, *mx = Pb + C * kStride;
    const bool has_b = job.b_mat != kAncestralNone;
    for (uint32_t i = threadIdx.x; i < C * S * S; i += blockDim.x) {
        const uint32_t c = i / (S * S), r = i % (S * S);
        Pa[c * kStride + r] = p_full[((uint64_t)job.a_mat * C + c) * (S * S) + r];
        if (has_b) Pb[c * kStride + r] = p_full[((uint64_t)job.b_mat * C + c) * (S * S) + r];
    }
    __syncthreads();
    // nucleotides: the threads of a site side by side, as its categories lie in memory; amino acids: a wave a category
    const uint32_t in_tile = S == 4 ? threadIdx.x / C : threadIdx.x % kTile, c = S == 4 ? threadIdx.x % C : threadIdx.x / kTile;
    const uint64_t site = (uint64_t)blockIdx.y * kTile + in_tile;
    const bool valid = site < Lc;
    double out[S];
    double m = 0.0;
    if (valid) {
        double v[S];
        load_vector<S>(part, masks, job.a_src, Lc, C, site, c, v);
        mat_vec<S>(Pa + c * kStride, v, out);
        if (has_b) {
            double f[S];
            load_vector<S>(part, masks, job.b_src, Lc, C, site, c, v);
            mat_vec<S>(Pb + c * kStride, v, f);
#pragma unroll
            for (uint32_t x = 0; x < S; ++x) out[x] = out[x] * f[x];
        }
#pragma unroll
        for (uint32_t x = 0; x < S; ++x)
            if (out[x] > m) m = out[x];
    }
    mx[in_tile * C + c] = m;
    __syncthreads();
    if (!valid) return;
    m = 0.0;
    for (uint32_t k = 0; k < C; ++k) {
        const double other = mx[in_tile * C + k];
        if (other > m) m = other;
    }
    if (m > 0.0) {
        int e = 0;
        (void)frexp(m, &e);
#pragma unroll
        for (uint32_t x = 0; x < S; ++x) out[x] = ldexp(out[x], -e);
    }
    double2 *dst = reinterpret_cast<double2 *>(part + (((uint64_t)job.out_slot * Lc + site) * C + c) * S);
#pragma unroll
    for (uint32_t x = 0; x < S / 2; ++x) dst[x] = make_double2(out[2 * x], out[2 * x + 1]);
}

template <uint32_t S>
__global__ __launch_bounds__(kTile *kAncestralMaxCategories) void down_kernel(const Job *__restrict__ jobs, double *__restrict__ part,
                                                                               const uint32_t *__restrict__ masks,
                                                                               const double *__restrict__ p_full, uint64_t Lc, uint32_t C)
{
    combine_tile<S>(jobs[blockIdx.x], part, masks, p_full, Lc, C);
}

template <uint32_t S>
__global__ __launch_bounds__(kTile *kAncestralMaxCategories) void up_kernel(const Job *__restrict__ jobs, double *__restrict__ part,
                                                                             const uint32_t *__restrict__ masks,
                                                                             const double *__restrict__ p_full, uint64_t Lc, uint32_t C)
{
    combine_tile<S>(jobs[blockIdx.x], part, masks, p_full, Lc, C);
}

// num[x] / Z rounded to float32, or a row of zeros (false)
template <uint32_t S>
__device__ inline bool write_row(const double (&num)[S], float *__restrict__ out)
{
    double Z = num[0];
#pragma unroll
    for (uint32_t x = 1; x < S; ++x) Z = Z + num[x];
    const bool alive = Z > 0.0 && Z <= 1.7976931348623157e308;
#pragma unroll
    for (uint32_t x = 0; x < S; ++x) out[x] = alive ? (float)(num[x] / Z) : 0.0f;
    return alive;
}

// Branch blockIdx.x, a site a thread.  out is [G][out_L][S] and the chunk's sites start at out_s0 of it.
template <uint32_t S>
__global__ __launch_bounds__(kTile) void ghost_kernel(const uint32_t *__restrict__ ghost_src, const double *__restrict__ part,
                                                      const uint32_t *__restrict__ masks, const double *__restrict__ p_half,
                                                      const double *__restrict__ p_pend, const double *__restrict__ weights,
                                                      const double *__restrict__ pi, uint64_t Lc, uint32_t C, uint32_t u_base,
                                                      uint32_t num_branches, uint32_t ghosts, float *__restrict__ out, uint64_t out_L,
                                                      uint64_t out_s0, unsigned long long *__restrict__ dead)
{
    const uint32_t b = blockIdx.x;
    const uint64_t site = (uint64_t)blockIdx.y * kTile + threadIdx.x;
    if (site >= Lc) return;
    const bool inner = ghosts != EPIK_AMD_GHOSTS_OUTER, outer = ghosts != EPIK_AMD_GHOSTS_INNER;
    const uint32_t src = ghost_src[b];
    double num[S], numb[S];
    for (uint32_t c = 0; c < C; ++c) {
        const double *h = p_half + ((uint64_t)b * C + c) * (S * S), *q = p_pend + ((uint64_t)b * C + c) * (S * S);
        const double wc = weights[c];
        double v[S], t[S], f[S];
        load_vector<S>(part, masks, src, Lc, C, site, c, v);
        mat_vec<S>(h, v, t);
        load_vector<S>(part, masks, u_base + b, Lc, C, site, c, v);
        mat_vec<S>(h, v, f);
#pragma unroll
        for (uint32_t x = 0; x < S; ++x) t[x] = pi[x] * (t[x] * f[x]);
#pragma unroll
        for (uint32_t x = 0; x < S; ++x) num[x] = c == 0 ? wc * t[x] : num[x] + wc * t[x];
        if (outer) {
#pragma unroll
            for (uint32_t y = 0; y < S; ++y) {
                double acc = t[0] * q[y];
#pragma unroll
                for (uint32_t x = 1; x < S; ++x) acc = acc + t[x] * q[x * S + y];
                numb[y] = c == 0 ? wc * acc : numb[y] + wc * acc;
            }
        }
    }
    unsigned long long zeroed = 0;
    if (inner && !write_row<S>(num, out + (((uint64_t)b * out_L) + out_s0 + site) * S)) ++zeroed;
    if (outer) {
        const uint64_t g = (ghosts == EPIK_AMD_GHOSTS_BOTH ? num_branches : 0) + (uint64_t)b;
        if (!write_row<S>(numb, out + ((g * out_L) + out_s0 + site) * S)) ++zeroed;
    }
    if (zeroed) atomicAdd(dead, zeroed);
}

// ---- host ---------------------------------------------------------------------------------------------------------

uint32_t source_of(const ancestral_tree &tree, uint32_t u)
{
    return tree.left[u] == kAncestralNone ? (tree.leaf_row[u] | kLeafFlag) : tree.inner_slot[u];
}

template <uint32_t S>
int run_chunk(epik_amd_ancestral *h, double *part, const uint32_t *d_masks, uint64_t Lc, uint32_t ghosts, float *out, uint64_t out_L,
              uint64_t out_s0)
{
    const uint32_t C = h->C;
    const double *p_full = h->d_tables, *p_half = p_full + (uint64_t)(h->N - 1) * C * S * S, *p_pend = p_half + (uint64_t)(h->N - 1) * C * S * S;
    const double *weights = p_pend + (uint64_t)(h->N - 1) * C * S * S, *pi = weights + C;
    const uint32_t tiles = (uint32_t)((Lc + kTile - 1) / kTile);
    const size_t lds = pass_lds_bytes<S>(C);
    for (const auto &[first, count] : h->down_levels)
        hipLaunchKernelGGL(down_kernel<S>, dim3(count, tiles), dim3(kTile * C), lds, h->stream, h->d_jobs + first, part, d_masks, p_full, Lc, C);
    for (const auto &[first, count] : h->up_levels)
        hipLaunchKernelGGL(up_kernel<S>, dim3(count, tiles), dim3(kTile * C), lds, h->stream, h->d_jobs + first, part, d_masks, p_full, Lc, C);
    hipLaunchKernelGGL(ghost_kernel<S>, dim3(h->N - 1, tiles), dim3(kTile), 0, h->stream, h->d_ghost_src, part, d_masks, p_half, p_pend, weights,
                       pi, Lc, C, h->n_inner, h->N - 1, ghosts, out, out_L, out_s0, h->d_dead);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

int posteriors_impl(epik_amd_ancestral *h, const uint32_t *masks, uint64_t L, uint32_t ghosts, float *post, uint32_t *branch_of,
                    uint64_t *dead_sites, bool on_device)
{
    if (!h) return fail_with(EPIK_AMD_ERR_INVALID, "null handle");
    std::string err;
    if (const int rc = ancestral_check_call(masks, L, ghosts, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
    if (!branch_of || (L && !post)) return fail_with(EPIK_AMD_ERR_INVALID, on_device ? "null device buffer" : "null host buffer");
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t G = ancestral_ghost_count(h->N, ghosts);
    std::vector<uint32_t> branches(G);
    ancestral_branch_of(h->N, ghosts, branches.data());
    if (on_device)
        HIP_TRY(hipMemcpy(branch_of, branches.data(), G * sizeof(uint32_t), hipMemcpyHostToDevice));
    else
        std::memcpy(branch_of, branches.data(), G * sizeof(uint32_t));
    HIP_TRY(hipMemsetAsync(h->d_dead, 0, sizeof(unsigned long long), h->stream));
    // the workspace: partials | masks | the posteriors of a chunk (host output only)
    const uint64_t slots = (uint64_t)h->n_inner + h->N - 1, cap = h->chunk_sites;
    double *part = reinterpret_cast<double *>(h->ws);
    uint32_t *d_masks = reinterpret_cast<uint32_t *>(h->ws + align_up(slots * cap * h->C * h->S * sizeof(double)));
    float *d_out = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(d_masks) + align_up((uint64_t)h->n_leaves * cap * sizeof(uint32_t)));
    for (uint64_t s0 = 0; s0 < L; s0 += cap) {
        const uint64_t Lc = std::min(cap, L - s0);
        HIP_TRY(hipMemcpy2DAsync(d_masks, Lc * sizeof(uint32_t), masks + s0, L * sizeof(uint32_t), Lc * sizeof(uint32_t), h->n_leaves,
                                 hipMemcpyHostToDevice, h->stream));
        float *out = on_device ? post : d_out;
        const uint64_t out_L = on_device ? L : Lc, out_s0 = on_device ? s0 : 0;
        if (const int rc = h->S == 4 ? run_chunk<4>(h, part, d_masks, Lc, ghosts, out, out_L, out_s0)
                                     : run_chunk<20>(h, part, d_masks, Lc, ghosts, out, out_L, out_s0);
            rc != EPIK_AMD_OK)
            return rc;
        if (!on_device)
            HIP_TRY(hipMemcpy2DAsync(post + s0 * h->S, L * h->S * sizeof(float), d_out, Lc * h->S * sizeof(float), Lc * h->S * sizeof(float), G,
                                     hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    unsigned long long dead = 0;
    HIP_TRY(hipMemcpyAsync(&dead, h->d_dead, sizeof dead, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (dead_sites) *dead_sites = dead;
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_ancestral_create(int device, const epik_amd_ancestral_desc *desc, uint64_t workspace_bytes, epik_amd_ancestral **handle)
{
    if (!handle || !desc) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *handle = nullptr;
    try {
        std::string err;
        ancestral_tree tree;
        if (const int rc = ancestral_check(*desc, tree, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail_with(EPIK_AMD_ERR_NO_DEVICE, "no HIP device");
        if (device < 0 || device >= count) return fail_with(EPIK_AMD_ERR_INVALID, "device " + std::to_string(device) + " does not exist");
        const uint32_t N = desc->num_nodes, S = desc->sigma, C = desc->num_categories;
        auto h = std::unique_ptr<epik_amd_ancestral, void (*)(epik_amd_ancestral *)>(new epik_amd_ancestral, epik_amd_ancestral_destroy);
        h->device = device, h->N = N, h->S = S, h->C = C, h->n_inner = tree.n_inner, h->n_leaves = tree.n_leaves;
        h->ws_bytes = workspace_bytes ? workspace_bytes : 4ull << 30;
        // a site: its partials, its masks, its posteriors of both ghost nodes of every branch (+ three alignments)
        const uint64_t slots = (uint64_t)tree.n_inner + N - 1;
        h->site_bytes = slots * C * S * sizeof(double) + (uint64_t)tree.n_leaves * sizeof(uint32_t) + 2ull * (N - 1) * S * sizeof(float);
        if (h->ws_bytes < h->site_bytes + 3 * 256)
            return fail_with(EPIK_AMD_ERR_INVALID, "one site of this tree needs a workspace of " + std::to_string(h->site_bytes + 3 * 256) +
                                                       " bytes, workspace_bytes is " + std::to_string(h->ws_bytes));
        h->chunk_sites = std::min<uint64_t>((h->ws_bytes - 3 * 256) / h->site_bytes, kMaxTiles * kTile);
        // the levels as jobs
        std::vector<Job> jobs;
        for (const auto &level : tree.down_levels) {
            h->down_levels.push_back({jobs.size(), (uint32_t)level.size()});
            for (const uint32_t v : level) {
                const uint32_t l = tree.left[v], r = tree.right[v];
                jobs.push_back(Job{tree.inner_slot[v], l, source_of(tree, l), r, source_of(tree, r)});
            }
        }
        for (const auto &level : tree.up_levels) {
            h->up_levels.push_back({jobs.size(), (uint32_t)level.size()});
            for (const uint32_t v : level) {
                const uint32_t p = (uint32_t)desc->parent[v], sib = tree.sibling[v];
                const bool at_root = p == N - 1;
                jobs.push_back(Job{tree.n_inner + v, sib, source_of(tree, sib), at_root ? kAncestralNone : p, at_root ? 0u : tree.n_inner + p});
            }
        }
        std::vector<uint32_t> ghost_src(N - 1);
        for (uint32_t b = 0; b + 1 < N; ++b) ghost_src[b] = source_of(tree, b);
        const auto fail = [&](hipError_t e, const char *what) { return fail_with(EPIK_AMD_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
        if (const hipError_t e = hipSetDevice(device); e != hipSuccess) return fail(e, "hipSetDevice");
        if (const hipError_t e = hipStreamCreate(&h->stream); e != hipSuccess) return fail(e, "hipStreamCreate");
        const uint64_t table = (uint64_t)(N - 1) * C * S * S;
        if (const hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->d_tables), (3 * table + C + S) * sizeof(double)); e != hipSuccess)
            return fail(e, "hipMalloc of the tables");
        if (const hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->d_jobs), jobs.size() * sizeof(Job)); e != hipSuccess) return fail(e, "hipMalloc");
        if (const hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->d_ghost_src), ghost_src.size() * sizeof(uint32_t)); e != hipSuccess)
            return fail(e, "hipMalloc");
        if (const hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->d_dead), sizeof(unsigned long long)); e != hipSuccess) return fail(e, "hipMalloc");
        if (const hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->ws), h->ws_bytes); e != hipSuccess) return fail(e, "hipMalloc of the workspace");
        const double *parts[5] = {desc->p_full, desc->p_half, desc->p_pend, desc->weights, desc->pi};
        const uint64_t sizes[5] = {table, table, table, C, S};
        uint64_t at = 0;
        for (int i = 0; i < 5; ++i) {
            if (const hipError_t e = hipMemcpy(h->d_tables + at, parts[i], sizes[i] * sizeof(double), hipMemcpyHostToDevice); e != hipSuccess)
                return fail(e, "hipMemcpy of the tables");
            at += sizes[i];
        }
        if (const hipError_t e = hipMemcpy(h->d_jobs, jobs.data(), jobs.size() * sizeof(Job), hipMemcpyHostToDevice); e != hipSuccess)
            return fail(e, "hipMemcpy");
        if (const hipError_t e = hipMemcpy(h->d_ghost_src, ghost_src.data(), ghost_src.size() * sizeof(uint32_t), hipMemcpyHostToDevice); e != hipSuccess)
            return fail(e, "hipMemcpy");
        *handle = h.release();
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("ancestral_create: ") + e.what());
    }
}

int epik_amd_ancestral_posteriors(epik_amd_ancestral *handle, const uint32_t *masks, uint64_t L, uint32_t ghosts, float *post,
                                  uint32_t *branch_of, uint64_t *dead_sites)
{
    try {
        return posteriors_impl(handle, masks, L, ghosts, post, branch_of, dead_sites, false);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("ancestral_posteriors: ") + e.what());
    }
}

int epik_amd_ancestral_posteriors_device(epik_amd_ancestral *handle, const uint32_t *masks, uint64_t L, uint32_t ghosts, void *d_post,
                                         void *d_branch_of, uint64_t *dead_sites)
{
    try {
        return posteriors_impl(handle, masks, L, ghosts, static_cast<float *>(d_post), static_cast<uint32_t *>(d_branch_of), dead_sites, true);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("ancestral_posteriors_device: ") + e.what());
    }
}

void epik_amd_ancestral_destroy(epik_amd_ancestral *handle)
{
    if (!handle) return;
    if (handle->device >= 0) {
        (void)hipSetDevice(handle->device);
        if (handle->stream) (void)hipStreamSynchronize(handle->stream);
        if (handle->ws) (void)hipFree(handle->ws);
        if (handle->d_tables) (void)hipFree(handle->d_tables);
        if (handle->d_jobs) (void)hipFree(handle->d_jobs);
        if (handle->d_ghost_src) (void)hipFree(handle->d_ghost_src);
        if (handle->d_dead) (void)hipFree(handle->d_dead);
        if (handle->stream) (void)hipStreamDestroy(handle->stream);
    }
    delete handle;
}

int epik_amd_ancestral_host(const epik_amd_ancestral_desc *desc, const uint32_t *masks, uint64_t L, uint32_t ghosts, uint32_t num_threads,
                            float *post, uint32_t *branch_of, uint64_t *dead_sites)
{
    if (!desc) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    try {
        std::string err;
        ancestral_tree tree;
        if (const int rc = ancestral_check(*desc, tree, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        if (const int rc = ancestral_check_call(masks, L, ghosts, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        if (!branch_of || (L && !post)) return fail_with(EPIK_AMD_ERR_INVALID, "null host buffer");
        ancestral_branch_of(desc->num_nodes, ghosts, branch_of);
        ancestral_rule_host(*desc, tree, masks, L, ghosts, num_threads, post, dead_sites);
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("ancestral_host: ") + e.what());
    }
}

int epik_amd_model_pmatrices(uint32_t sigma, const double *exchange, const double *pi, const double *times, uint64_t n, double *out)
{
    try {
        std::string err;
        if (const int rc = model_pmatrices(sigma, exchange, pi, times, n, out, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("model_pmatrices: ") + e.what());
    }
}

int epik_amd_model_gamma_rates(double alpha, uint32_t num_categories, double *rates)
{
    try {
        std::string err;
        if (const int rc = model_gamma_rates(alpha, num_categories, rates, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("model_gamma_rates: ") + e.what());
    }
}

}  // extern "C"
