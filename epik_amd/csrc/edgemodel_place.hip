// edgemodel_place.hip -- the edge model of a cohort's samples on the device: a sequential linear model per branch, of its mass
// and of its imbalance, with factors and numeric covariates, each term tested after the ones before it, by permutation, with the
// edge test's single-step max-statistic adjustment.  epik_amd_cohort_edgemodel_device / _edgemodel / _edgemodel_host and their
// _strata forms (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h after the Mantel rule (DESIGN.md 3.28;
// epik_amd/host/cohort.cpp: edgemodel_records is the same rule on the CPU).  Every sum is a sequential chain from +0.0 in one
// lane (__dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn; the file is built with -ffp-contract=off as well).  No MFMA and no
// fused multiply-add: the chains have a fixed order and every product is rounded.  A maximum of doubles that are >= +0.0 is a
// maximum of their bit patterns.  NA is stored as its bit pattern and never computed.
//
// cohort_mass_plane_enqueue (correlation_place.hip) leaves T_s, the planes C and B, and xm as a plane [b][Sp].  Then
//
//   model_terms_kernel, model_basis_kernel, model_strata_kernel
//                               the sequential model's (model_basis.hpp): the list of the complete cases, the basis Q[L][64],
//                               df, R, df_res, the aliased bytes, and with strata the tables of the list.
//   edgemodel_observed_kernel   a workgroup a branch: xm and xi over the list (branch_vectors without ranks), in LDS or, beyond
//                               kLdsPositions samples, in the workgroup's slice of global memory; a wave a family centres its
//                               vector; the deviations go to the plane D[b][f][Sp]; a lane a (family, column) walks the chain
//                               s_c of the identity; a lane a family writes the records of every term and phi_k(sigma_0) into a
//                               table.  A branch with a defined family joins the list of the branches to permute.
//   edgemodel_arrange_kernel    a workgroup a permutation of the chunk: sigma_p (permutation_rank, or permutation_arrangement
//                               with strata) into SIG[i][k], permutation-fastest.
//   edgemodel_gather_kernel     the arranged basis of the chunk, once for every listed branch: QS[i][k * Rb + c] = Q[sigma_k(i)][c],
//                               chain-fastest, so that the hot kernel's staging reads lines.  Rb: the columns the host can bound.
//   edgemodel_chains_kernel     the hot kernel: D[rows][L] . QS[L][chains] in a fixed order.  A workgroup owns a tile of kRows
//                               rows (kTileBranches listed branches x 2 families) times kTileCols chains (whole permutations:
//                               kTileCols / Rb of them) and walks i ascending in slabs of kSlab, a slab of D and one of QS in
//                               LDS; a lane keeps kRegRows x kRegCols chains in registers, so one LDS read feeds several
//                               multiply-adds.  A chain is i ascending whatever the tiling: the bits depend on neither the tile
//                               sizes nor the grid.  Then s goes to LDS (over the QS slab) and a lane a (row, permutation)
//                               forms SS_k, SS_res and phi_k of every term, writes stat, counts phi >= phi_0 and takes the
//                               maximum of a (term, family, permutation) over the tile's branches in LDS; one vector atomic a
//                               (row, term) and one a (term, family, permutation) leave the workgroup.
//   edgemodel_finish_kernel     max_at_least, p and p_adj of every defined (term, branch, family); NA into stat where undefined; max.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"
#include "model_basis.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kTerms = kModelTerms, kColumns = kModelColumns, kPitch = kModelPitch;
constexpr uint32_t kFamilies = EPIK_AMD_EDGEMODEL_FAMILIES;
constexpr uint32_t kLdsPositions = kCohortLdsSamples;  // the most samples whose vectors stay in LDS in the observed pass
constexpr uint32_t kTileBranches = 16;                 // listed branches a tile of the hot kernel
constexpr uint32_t kRows = kTileBranches * kFamilies;  // ... its rows: a (branch, family) each
constexpr uint32_t kTileCols = 128;                    // ... its chains: kTileCols / Rb whole permutations
constexpr uint32_t kSlab = 32;                         // positions staged at a time
constexpr uint32_t kRegRows = 4, kRegCols = 4;         // a lane's register block
constexpr uint32_t kRowPitch = kRows + 2;              // doubles a position of the D slab (the staging writes spread over the banks)
constexpr uint32_t kChunkTiles = 32;                   // tiles of chains a chunk of permutations: 4 096 chains at the most
constexpr uint32_t kGeneralBlocks = 256;               // workgroups of the observed kernel's general path: each has a slice
constexpr uint64_t kManyBlocks = 65536;

static_assert(sizeof(epik_amd_edgemodel_family) == 72 && sizeof(epik_amd_edgemodel) == 144 && sizeof(epik_amd_edgemodel_info) == 152);
static_assert(kFamilies == 2 && kBlock == 256 && kWave == 64 && kFamilies * kColumns <= kBlock);
static_assert((kRows / kRegRows) * (kTileCols / kRegCols) == kBlock, "a lane a register block, the blocks cover the tile");
static_assert(kRows * kTileCols <= kSlab * kTileCols, "the sums of a tile fit over the slab of the arranged basis");
static_assert(kColumns <= kTileCols && kBlock % kSlab == 0 && kBlock % kTileCols == 0 && kRowPitch % 2 == 0);

struct EdgemodelSpace {
    double *D;         // [N][2][Sp]: the deviations
    double *QS;        // [Sp][chains]: the arranged basis of a chunk, chains = min(chunk_perms, P + 1) * Rb <= 4 096
    double *Q;         // [Sp][kPitch]: the basis, a position a row
    double *v;         // [Sp]: the column at work
    double *val;       // [T][Sp]: the values by sample
    double *scratch;   // [slices][2][Sp]: the vectors of a workgroup of the general path
    double *sxx;       // [N][2]
    double *phi0;      // [T][N][2]: phi_k of the identity
    uint64_t *mmax;    // [T][2][P + 1]: the bit patterns of Mmax
    ModelMeta *meta;
    uint32_t *SIG;     // [Sp][perms]: sigma of a chunk, permutation-fastest, perms = min(chunk_perms, P + 1)
    uint32_t *lab;     // [T][Sp]: the labels by sample, `missing` for a sample that is no complete case
    uint32_t *idx;     // [T][Sp]: the samples of the positions (every term's list is the same)
    uint32_t *defined; // [N]: bit f: family f of the branch has sxx > 0 under a testable design
    uint32_t *active;  // [N] the branches to permute, then their number, then the defined branches of the two families
    uint8_t *lam;      // [T][Sp]: the groups of the positions
    uint32_t *strata;  // with strata only: [Sp], the strata by sample
    uint32_t *hs, *home;  // ... and [Sp]: the strata of the positions, and the positions by (stratum, position)
};

size_t edgemodel_space(void *base, uint32_t N, uint32_t padded, uint32_t T, uint32_t P, uint32_t chains, uint32_t perms, uint32_t slices,
                       bool strata, EdgemodelSpace *sp)
{
    Carver c(base);
    const EdgemodelSpace parts{.D = c.take<double>((size_t)N * kFamilies * padded),
                               .QS = c.take<double>((size_t)padded * chains),
                               .Q = c.take<double>((size_t)padded * kPitch),
                               .v = c.take<double>(padded),
                               .val = c.take<double>((size_t)T * padded),
                               .scratch = c.take<double>((size_t)slices * kFamilies * padded),
                               .sxx = c.take<double>((size_t)N * kFamilies),
                               .phi0 = c.take<double>((size_t)T * N * kFamilies),
                               .mmax = c.take<uint64_t>((size_t)T * kFamilies * ((size_t)P + 1)),
                               .meta = c.take<ModelMeta>(1),
                               .SIG = c.take<uint32_t>((size_t)padded * perms),
                               .lab = c.take<uint32_t>((size_t)T * padded),
                               .idx = c.take<uint32_t>((size_t)T * padded),
                               .defined = c.take<uint32_t>(N),
                               .active = c.take<uint32_t>((size_t)N + 1 + kFamilies),
                               .lam = c.take<uint8_t>((size_t)T * padded),
                               .strata = c.take<uint32_t>(strata ? padded : 0),
                               .hs = c.take<uint32_t>(strata ? padded : 0),
                               .home = c.take<uint32_t>(strata ? padded : 0)};
    if (sp) *sp = parts;
    return c.bytes();
}

struct EdgemodelArgs {
    const double *X, *planes;
    const uint32_t *first;
    EdgemodelSpace sp;
    epik_amd_edgemodel *out;        // [T][N]
    epik_amd_edgemodel_info *info;
    double *stat;                   // [T][2][N][P + 1], or null
    double *max;                    // [T][2][P + 1], or null
    uint64_t seed;
    uint32_t num_terms, num_branches, padded, num_permutations;
    uint32_t Rb;                    // the chains a permutation takes in QS: the host's bound of R, at least 1
    uint32_t tile_perms, chunk_perms;  // kTileCols / Rb, and kChunkTiles times that
    uint32_t sig_pitch, qs_pitch;      // the permutations and the chains a position of SIG and of QS: min(chunk_perms, P + 1), times Rb
    uint32_t p0, np;                // the chunk: the permutations p0 .. p0 + np - 1
};

// phi_k of the rule from SS_k and SS_res
__device__ inline double phi_of(double ss, double res)
{
    if (res > 0.0) return __ddiv_rn(ss, __dadd_rn(ss, res));
    return ss > 0.0 ? 1.0 : 0.0;
}

// SS_k: the chain of s_c * s_c over the accepted columns [first, first + df) of a term
__device__ inline double term_ss(const double *s, uint32_t first, uint32_t df)
{
    double ss = 0.0;
    for (uint32_t w = 0; w < df; ++w) ss = __dadd_rn(ss, __dmul_rn(s[first + w], s[first + w]));
    return ss;
}

template <bool kLds>
__global__ __launch_bounds__(kBlock) void edgemodel_observed_kernel(const EdgemodelArgs a)
{
    __shared__ double lds_vec[kLds ? kFamilies * kLdsPositions : 1];
    __shared__ double sxx_of[kFamilies], s_of[kFamilies][kColumns];
    __shared__ ModelMeta m;
    const uint32_t tid = threadIdx.x, N = a.num_branches, padded = a.padded, T = a.num_terms;
    if (tid == 0) m = *a.sp.meta;
    __syncthreads();
    const uint32_t pitch = kLds ? kLdsPositions : padded;
    double *vec = kLds ? lds_vec : a.sp.scratch + (uint64_t)blockIdx.x * kFamilies * padded;
    const double *C = a.planes, *B = a.planes + (uint64_t)N * padded;
    const uint32_t L = m.L, R = m.R;
    const bool testable = m.df_res >= 1 && R >= 1;  // (uniform, as is every condition around a barrier below)
    if (blockIdx.x == 0 && tid == 0) {
        epik_amd_edgemodel_info info{L, T, m.C, R, m.df_res, {}, {}};
        for (uint32_t t = 0; t < T; ++t) info.df[t] = m.df[t], info.term_columns[t] = m.columns[t];
        *a.info = info;
    }
    for (uint32_t b = blockIdx.x; b < N; b += gridDim.x) {
        const bool inner = a.first[b] < b;
        const uint32_t nf = inner ? kFamilies : 1;
        if (testable) {
            branch_vectors<kLds, false>(a.X + (uint64_t)b * padded, C + (uint64_t)b * padded, B + (uint64_t)b * padded, a.sp.idx, L, inner, vec,
                                        pitch);
            if (tid % kWave == 0 && tid / kWave < nf) sxx_of[tid / kWave] = centre(vec + (tid / kWave) * pitch, L);  // a wave a family
            __syncthreads();
            for (uint32_t f = 0; f < kFamilies; ++f) {
                double *row = a.sp.D + ((uint64_t)b * kFamilies + f) * padded;
                for (uint32_t i = tid; i < L; i += kBlock) row[i] = f < nf ? vec[f * pitch + i] : 0.0;
            }
            if (tid < nf * R) {
                const uint32_t f = tid / R, c = tid % R;
                const double *d = vec + f * pitch;
                double acc = 0.0;
#pragma unroll 4
                for (uint32_t i = 0; i < L; ++i) acc = __dadd_rn(acc, __dmul_rn(a.sp.Q[(uint64_t)i * kPitch + c], d[i]));
                s_of[f][c] = acc;
            }
            __syncthreads();
        }
        if (tid < kFamilies) {
            const uint32_t f = tid;
            const double sxx = testable && f < nf ? sxx_of[f] : 0.0;
            const bool defined = sxx > 0.0;
            double res = 0.0;
            if (defined) {
                double model = 0.0;
                for (uint32_t t = 0; t < T; ++t) model = __dadd_rn(model, term_ss(s_of[f], m.first[t], m.df[t]));
                res = __dsub_rn(sxx, model);
                atomicAdd(a.sp.active + N + 1 + f, 1u);
            }
            for (uint32_t t = 0; t < T; ++t) {
                epik_amd_edgemodel_family fam{na_value(), na_value(), na_value(), na_value(), na_value(), na_value(), 0, 0, 0, 0};
                double phi = 0.0;
                if (defined && m.df[t]) {
                    const double ss = term_ss(s_of[f], m.first[t], m.df[t]);
                    phi = phi_of(ss, res);
                    fam.ss = ss, fam.r2 = __ddiv_rn(ss, sxx), fam.partial_r2 = phi;
                    if (res > 0.0) fam.f = __ddiv_rn(__ddiv_rn(ss, (double)m.df[t]), __ddiv_rn(res, (double)m.df_res));
                    if (m.df[t] == 1) {
                        const double s = s_of[f][m.first[t]];
                        fam.sign = s > 0.0 ? 1 : s < 0.0 ? -1 : 0;
                    }
                }
                a.out[(uint64_t)t * N + b].family[f] = fam;
                a.sp.phi0[((uint64_t)t * N + b) * kFamilies + f] = phi;
            }
            a.sp.sxx[(uint64_t)b * kFamilies + f] = sxx;
            const uint32_t mask = (uint32_t)__ballot(defined) & 0x3u;  // (the two lanes are the first of wave 0)
            if (f == 0) {
                a.sp.defined[b] = mask;
                if (mask) a.sp.active[atomicAdd(a.sp.active + N, 1u)] = b;
            }
        }
        __syncthreads();  // (the vectors and the sums are written again)
    }
}

template <bool kStrata>
__global__ __launch_bounds__(kBlock) void edgemodel_arrange_kernel(const EdgemodelArgs a)
{
    __shared__ uint64_t tile[kCohortKeyTile];
    const uint32_t tid = threadIdx.x, L = a.sp.meta->L;
    if (a.sp.active[a.num_branches] == 0) return;  // (uniform: no branch to permute)
    for (uint32_t k = blockIdx.x; k < a.np; k += gridDim.x) {
        const uint32_t p = a.p0 + k;
        for (uint32_t base = 0; base < L; base += kBlock) {  // (every lane calls: it has barriers)
            const uint32_t i = base + tid;
            uint32_t rank;  // (permutation 0 is the identity)
            if constexpr (kStrata) {
                __shared__ uint32_t htile[kCohortKeyTile];
                rank = permutation_arrangement(a.seed, p, i, L, tile, htile, a.sp.hs, a.sp.home);
            } else {
                rank = permutation_rank(a.seed, p, i, L, tile);
            }
            if (i < L) a.sp.SIG[(uint64_t)i * a.sig_pitch + k] = rank;  // (k < np <= sig_pitch)
        }
    }
}

__global__ __launch_bounds__(kBlock) void edgemodel_gather_kernel(const EdgemodelArgs a)
{
    if (a.sp.active[a.num_branches] == 0) return;
    const uint32_t L = a.sp.meta->L, R = a.sp.meta->R, Rb = a.Rb;
    const uint64_t width = (uint64_t)a.np * Rb, cells = (uint64_t)L * width;  // (width <= qs_pitch)
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t i = (uint32_t)(e / width), j = (uint32_t)(e - (uint64_t)i * width), k = j / Rb, c = j % Rb;
        if (c < R) a.sp.QS[(uint64_t)i * a.qs_pitch + j] = a.sp.Q[(uint64_t)a.sp.SIG[(uint64_t)i * a.sig_pitch + k] * kPitch + c];  // (sigma < L)
    }
}

__global__ __launch_bounds__(kBlock) void edgemodel_chains_kernel(const EdgemodelArgs a)
{
    __shared__ __align__(16) double Ds[kSlab * kRowPitch];
    __shared__ __align__(16) double Qt[kSlab * kTileCols];       // the slab of QS; afterwards the sums s[kRows][kTileCols]
    __shared__ unsigned long long mx[kTileCols][kFamilies];      // [o * tile_perms + k][f]: the maximum over the tile's branches
    __shared__ uint32_t cnt[kRows][kTerms];                      // [row][o]: the permutations that reach the observed phi
    __shared__ uint32_t term_of[kTerms], tested;                 // the terms with df >= 1, in order
    __shared__ ModelMeta m;
    const uint32_t tid = threadIdx.x, N = a.num_branches, padded = a.padded, P = a.num_permutations;
    const uint32_t listed = a.sp.active[N];
    if (listed == 0) return;  // (uniform)
    if (tid == 0) {
        m = *a.sp.meta;
        uint32_t nd = 0;
        for (uint32_t t = 0; t < a.num_terms; ++t)
            if (m.df[t]) term_of[nd++] = t;
        tested = nd;
    }
    __syncthreads();
    const uint32_t L = m.L, R = m.R, Rb = a.Rb, tile_perms = a.tile_perms, nd = tested;
    const uint32_t width = tile_perms * Rb;  // the chains of a tile that carry a permutation (<= kTileCols)
    const uint64_t row_len = (uint64_t)P + 1;
    const uint32_t col_tiles = (a.np + tile_perms - 1) / tile_perms, row_tiles = (listed + kTileBranches - 1) / kTileBranches;
    const uint32_t tr = tid / (kTileCols / kRegCols), tc = tid % (kTileCols / kRegCols);  // the lane's register block
    const uint32_t stage_j = tid % kTileCols, stage_row = tid / kSlab, stage_i = tid % kSlab;
    for (uint32_t tile = blockIdx.x; tile < row_tiles * col_tiles; tile += gridDim.x) {
        const uint32_t at0 = tile / col_tiles * kTileBranches, k0 = tile % col_tiles * tile_perms, j0 = k0 * Rb;
        for (uint32_t e = tid; e < kRows * kTerms; e += kBlock) cnt[e / kTerms][e % kTerms] = 0;
        for (uint32_t e = tid; e < kTileCols * kFamilies; e += kBlock) mx[e / kFamilies][e % kFamilies] = 0;
        // the chain of this lane's staging column: a column of a permutation of the chunk, below R
        const bool stage_live = stage_j < width && k0 + stage_j / Rb < a.np && stage_j % Rb < R;
        double acc[kRegRows][kRegCols];
#pragma unroll
        for (uint32_t r = 0; r < kRegRows; ++r)
#pragma unroll
            for (uint32_t c = 0; c < kRegCols; ++c) acc[r][c] = 0.0;
        for (uint32_t i0 = 0; i0 < L; i0 += kSlab) {  // ascending: the rule's order
            const uint32_t ni = min(kSlab, L - i0);
            __syncthreads();  // (the slabs are written again)
#pragma unroll
            for (uint32_t it = 0; it < kRows * kSlab / kBlock; ++it) {
                const uint32_t row = stage_row + it * (kBlock / kSlab), at = at0 + row / kFamilies;
                double v = 0.0;
                if (at < listed && stage_i < ni) v = a.sp.D[((uint64_t)a.sp.active[at] * kFamilies + row % kFamilies) * padded + i0 + stage_i];
                Ds[stage_i * kRowPitch + row] = v;
            }
#pragma unroll
            for (uint32_t it = 0; it < kSlab * kTileCols / kBlock; ++it) {
                const uint32_t ii = tid / kTileCols + it * (kBlock / kTileCols);
                double v = 0.0;
                if (stage_live && ii < ni) v = a.sp.QS[(uint64_t)(i0 + ii) * a.qs_pitch + j0 + stage_j];
                Qt[ii * kTileCols + stage_j] = v;
            }
            __syncthreads();
            // (beyond ni both slabs hold +0.0: a chain from +0.0 never holds -0.0, so adding +0.0 leaves its bits)
#pragma unroll 8
            for (uint32_t ii = 0; ii < kSlab; ++ii) {
                double d[kRegRows], q[kRegCols];
#pragma unroll
                for (uint32_t r = 0; r < kRegRows; ++r) d[r] = Ds[ii * kRowPitch + tr * kRegRows + r];
#pragma unroll
                for (uint32_t c = 0; c < kRegCols; ++c) q[c] = Qt[ii * kTileCols + tc * kRegCols + c];
#pragma unroll
                for (uint32_t r = 0; r < kRegRows; ++r)
#pragma unroll
                    for (uint32_t c = 0; c < kRegCols; ++c) acc[r][c] = __dadd_rn(acc[r][c], __dmul_rn(q[c], d[r]));
            }
        }
        __syncthreads();  // (every lane has read the last slab: the sums take its place)
#pragma unroll
        for (uint32_t r = 0; r < kRegRows; ++r)
#pragma unroll
            for (uint32_t c = 0; c < kRegCols; ++c) Qt[(tr * kRegRows + r) * kTileCols + tc * kRegCols + c] = acc[r][c];
        __syncthreads();
        for (uint32_t e = tid; e < kRows * tile_perms; e += kBlock) {
            const uint32_t row = e / tile_perms, kk = e % tile_perms, at = at0 + row / kFamilies, f = row % kFamilies, k = k0 + kk;
            if (at >= listed || k >= a.np) continue;
            const uint32_t b = a.sp.active[at], p = a.p0 + k;
            if (!((a.sp.defined[b] >> f) & 1u)) continue;
            const double *s = Qt + row * kTileCols + kk * Rb;  // (kk * Rb + R <= width)
            double model = 0.0;
            for (uint32_t o = 0; o < nd; ++o) model = __dadd_rn(model, term_ss(s, m.first[term_of[o]], m.df[term_of[o]]));  // (a term without columns adds +0.0)
            const double res = __dsub_rn(a.sp.sxx[(uint64_t)b * kFamilies + f], model);
            for (uint32_t o = 0; o < nd; ++o) {
                const uint32_t t = term_of[o];
                const double phi = phi_of(term_ss(s, m.first[t], m.df[t]), res);
                if (a.stat) a.stat[(((uint64_t)t * kFamilies + f) * N + b) * row_len + p] = phi;
                atomicMax(&mx[o * tile_perms + kk][f], (unsigned long long)__double_as_longlong(phi));  // (o * tile_perms + kk < kTileCols)
                if (p >= 1 && phi >= a.sp.phi0[((uint64_t)t * N + b) * kFamilies + f]) atomicAdd(&cnt[row][o], 1u);
            }
        }
        __syncthreads();
        for (uint32_t e = tid; e < kRows * nd; e += kBlock) {
            const uint32_t row = e / nd, o = e % nd, at = at0 + row / kFamilies;
            const uint32_t count = cnt[row][o];
            if (count)  // (a count is above 0 only for a listed row)
                atomicAdd(reinterpret_cast<unsigned long long *>(&a.out[(uint64_t)term_of[o] * N + a.sp.active[at]].family[row % kFamilies].at_least),
                          (unsigned long long)count);
        }
        for (uint32_t e = tid; e < nd * tile_perms * kFamilies; e += kBlock) {
            const uint32_t cell = e / kFamilies, f = e % kFamilies, o = cell / tile_perms, k = k0 + cell % tile_perms;
            const unsigned long long most = mx[cell][f];
            if (most && k < a.np)
                atomicMax(reinterpret_cast<unsigned long long *>(a.sp.mmax + ((uint64_t)term_of[o] * kFamilies + f) * row_len + a.p0 + k), most);
        }
        __syncthreads();  // (the tables are zeroed again)
    }
}

__global__ __launch_bounds__(kBlock) void edgemodel_finish_kernel(const EdgemodelArgs a)
{
    const uint32_t N = a.num_branches, P = a.num_permutations, T = a.num_terms;
    const uint64_t row = (uint64_t)P + 1, units = (uint64_t)T * N * kFamilies;
    const uint64_t start = (uint64_t)blockIdx.x * kBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBlock;
    const double *mmax = reinterpret_cast<const double *>(a.sp.mmax);
    const uint32_t *df = a.sp.meta->df;
    for (uint64_t e = start; e < units; e += stride) {
        const uint32_t f = (uint32_t)(e % kFamilies), b = (uint32_t)(e / kFamilies % N), t = (uint32_t)(e / kFamilies / N);
        if (!df[t] || !((a.sp.defined[b] >> f) & 1u)) continue;
        epik_amd_edgemodel_family *fam = &a.out[(uint64_t)t * N + b].family[f];
        const double phi = fam->partial_r2;
        const double *mm = mmax + ((uint64_t)t * kFamilies + f) * row;
        uint64_t count = 0;
#pragma unroll 4
        for (uint32_t p = 1; p <= P; ++p) count += mm[p] >= phi;
        fam->max_at_least = count;
        fam->p = __ddiv_rn((double)(1 + fam->at_least), (double)(P + 1));
        fam->p_adj = __ddiv_rn((double)(1 + count), (double)(P + 1));
    }
    if (a.max)
        for (uint64_t e = start; e < (uint64_t)T * kFamilies * row; e += stride) {
            const uint64_t tf = e / row;  // t * 2 + f
            a.max[e] = df[tf / kFamilies] && a.sp.active[N + 1 + tf % kFamilies] ? mmax[e] : na_value();
        }
    if (a.stat)
        for (uint64_t e = start; e < units * row; e += stride) {
            const uint64_t tfb = e / row, tf = tfb / N;  // (t * 2 + f) * N + b
            if (!(df[tf / kFamilies] && ((a.sp.defined[tfb % N] >> (tf % kFamilies)) & 1u))) a.stat[e] = na_value();
        }
}

int check_arguments(const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t S, uint32_t T, uint32_t P)
{
    std::string err;
    return rule_result(model_arguments_valid(kind, labels, values, S, T, P, err), err);
}

int terms_valid(uint32_t T)
{
    if (T < 1 || T > kTerms) return fail_with(EPIK_AMD_ERR_INVALID, "num_terms = " + std::to_string(T) + " is outside [1, 16]");
    return EPIK_AMD_OK;
}

int edgemodel_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind, const uint32_t *labels,
                          const double *values, const uint32_t *strata, uint32_t T, uint32_t P, uint64_t seed, void *d_out, void *d_info,
                          void *d_stat, void *d_max, void *d_aliased, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(terms_valid(T));
    COHORT_TRY(check_present(tree, kind, labels, values, d_out, d_info, d_aliased));
    const uint32_t S = cohort->num_samples, N = cohort->num_branches, padded = cohort_padded_samples(cohort);
    COHORT_TRY(check_arguments(kind, labels, values, S, T, P));
    const uint32_t *d_first = nullptr;
    const double *d_X = nullptr;
    // (the checks of the tree; the device drained of every call before: nothing reads the workspace)
    COHORT_TRY(cohort_mass_plane_enqueue(cohort, tree, stream, &d_first, &d_X));
    const bool lds = lds_switch("EPIK_AMD_EDGEMODEL_LDS", S, kLdsPositions);  // (=0, tests: the general path whatever S)
    const dim3 observed = cohort_grid(cohort, N, lds ? kManyBlocks : kGeneralBlocks);
    const uint32_t slices = lds ? 0 : observed.x;
    // the chains a permutation takes in QS: the columns as the rule counts them, at least R (<= 64: the arguments were checked)
    const uint32_t Rb = (uint32_t)std::max<size_t>(1, model_design_columns(kind, labels, S, T));
    const uint32_t tile_perms = kTileCols / Rb, chunk_perms = kChunkTiles * tile_perms;
    const uint32_t sig_pitch = (uint32_t)std::min<uint64_t>(chunk_perms, (uint64_t)P + 1), qs_pitch = sig_pitch * Rb;  // (a small P: a small chunk)
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceEdgemodel,
                                   edgemodel_space(nullptr, N, padded, T, P, qs_pitch, sig_pitch, slices, strata != nullptr, nullptr)));
    EdgemodelSpace sp;
    edgemodel_space(cohort->space[kSpaceEdgemodel].d, N, padded, T, P, qs_pitch, sig_pitch, slices, strata != nullptr, &sp);
    if (strata) COHORT_TRY(upload_strata(strata, S, padded, sp.strata));
    ModelKinds kinds{};
    size_t bound = 0;
    COHORT_TRY(model_design_upload(kind, labels, values, S, T, padded, sp.lab, sp.val, kinds, bound));
    const uint64_t row = (uint64_t)P + 1;
    HIP_TRY(hipMemsetAsync(sp.meta, 0, sizeof(ModelMeta), stream));
    HIP_TRY(hipMemsetAsync(sp.Q, 0, (size_t)padded * kPitch * sizeof(double), stream));
    HIP_TRY(hipMemsetAsync(sp.active + N, 0, (1 + kFamilies) * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(sp.mmax, 0, (size_t)T * kFamilies * row * sizeof(uint64_t), stream));
    hipLaunchKernelGGL(model_terms_kernel, cohort_grid(cohort, T, kTerms), dim3(kWave), 0, stream, cohort->d_total, sp.lab, S, padded, T, sp.idx,
                       sp.lam, sp.meta);
    if (strata) hipLaunchKernelGGL(model_strata_kernel, dim3(1), dim3(kBlock), 0, stream, sp.strata, sp.idx, sp.meta, sp.hs, sp.home);
    hipLaunchKernelGGL(model_basis_kernel, dim3(1), dim3(kBlock), 0, stream, kinds, T, padded, sp.val, sp.idx, sp.lam, sp.v, sp.Q, sp.meta,
                       static_cast<uint8_t *>(d_aliased));
    EdgemodelArgs args{d_X, cohort->d_planes, d_first, sp, static_cast<epik_amd_edgemodel *>(d_out),
                       static_cast<epik_amd_edgemodel_info *>(d_info), static_cast<double *>(d_stat), static_cast<double *>(d_max), seed,
                       T, N, padded, P, Rb, tile_perms, chunk_perms, sig_pitch, qs_pitch, 0, 0};
    if (lds) hipLaunchKernelGGL((edgemodel_observed_kernel<true>), observed, dim3(kBlock), 0, stream, args);
    else hipLaunchKernelGGL((edgemodel_observed_kernel<false>), observed, dim3(kBlock), 0, stream, args);
    for (uint64_t p0 = 0; p0 < row; p0 += args.chunk_perms) {
        args.p0 = (uint32_t)p0, args.np = (uint32_t)std::min<uint64_t>(args.chunk_perms, row - p0);
        const dim3 arrange = cohort_grid(cohort, args.np, kManyBlocks);
        if (strata) hipLaunchKernelGGL(edgemodel_arrange_kernel<true>, arrange, dim3(kBlock), 0, stream, args);
        else hipLaunchKernelGGL(edgemodel_arrange_kernel<false>, arrange, dim3(kBlock), 0, stream, args);
        hipLaunchKernelGGL(edgemodel_gather_kernel, cohort_grid_per(cohort, (uint64_t)padded * args.np * Rb, kBlock, kManyBlocks), dim3(kBlock), 0,
                           stream, args);
        const uint64_t col_tiles = (args.np + args.tile_perms - 1) / args.tile_perms, row_tiles = (N + kTileBranches - 1) / kTileBranches;
        hipLaunchKernelGGL(edgemodel_chains_kernel, cohort_grid(cohort, col_tiles * row_tiles, kManyBlocks), dim3(kBlock), 0, stream, args);
    }
    const uint64_t units = (uint64_t)T * N * kFamilies;
    const uint64_t finish = d_stat ? units * row : std::max<uint64_t>(units, d_max ? (uint64_t)T * kFamilies * row : 0);
    hipLaunchKernelGGL(edgemodel_finish_kernel, cohort_grid_per(cohort, finish, kBlock, kManyBlocks), dim3(kBlock), 0, stream, args);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_edgemodel_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind, const uint32_t *labels,
                                     const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed, void *d_out,
                                     void *d_info, void *d_stat, void *d_max, void *d_aliased, void *stream)
{
    return epik_amd_cohort_edgemodel_strata_device(cohort, tree, kind, labels, values, num_terms, num_permutations, seed, d_out, d_info,
                                                   d_stat, d_max, d_aliased, stream, nullptr);
}

int epik_amd_cohort_edgemodel_strata_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind,
                                            const uint32_t *labels, const double *values, uint32_t num_terms, uint32_t num_permutations,
                                            uint64_t seed, void *d_out, void *d_info, void *d_stat, void *d_max, void *d_aliased,
                                            void *stream, const uint32_t *strata)
{
    return guarded("cohort_edgemodel_device", [&]() -> int {
        return edgemodel_device_impl(cohort, tree, kind, labels, values, strata, num_terms, num_permutations, seed, d_out, d_info, d_stat,
                                     d_max, d_aliased, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_edgemodel(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind, const uint32_t *labels,
                              const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                              epik_amd_edgemodel *out, epik_amd_edgemodel_info *info, double *stat, double *max, uint8_t *aliased)
{
    return epik_amd_cohort_edgemodel_strata(cohort, tree, kind, labels, values, num_terms, num_permutations, seed, out, info, stat, max,
                                            aliased, nullptr);
}

int epik_amd_cohort_edgemodel_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind, const uint32_t *labels,
                                     const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                                     epik_amd_edgemodel *out, epik_amd_edgemodel_info *info, double *stat, double *max, uint8_t *aliased,
                                     const uint32_t *strata)
{
    return guarded("cohort_edgemodel", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(terms_valid(num_terms));
        COHORT_TRY(check_present(tree, kind, labels, values, out, info, aliased));
        COHORT_TRY(check_arguments(kind, labels, values, cohort->num_samples, num_terms, num_permutations));
        const size_t row = (size_t)num_permutations + 1, N = cohort->num_branches, T = num_terms;
        const size_t out_bytes = T * N * sizeof(epik_amd_edgemodel);
        const size_t stat_bytes = T * kFamilies * N * row * sizeof(double);
        const size_t max_bytes = T * kFamilies * row * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult r, s, m;
        COHORT_TRY(r.alloc(out_bytes + sizeof(epik_amd_edgemodel_info) + kColumns));  // the records | the info block | aliased
        COHORT_TRY(s.alloc(stat_bytes, stat != nullptr));
        COHORT_TRY(m.alloc(max_bytes, max != nullptr));
        COHORT_TRY(edgemodel_device_impl(cohort, tree, kind, labels, values, strata, num_terms, num_permutations, seed, r.d, r.at(out_bytes),
                                         s.d, m.d, r.at(out_bytes + sizeof(epik_amd_edgemodel_info)), nullptr));
        COHORT_TRY(r.copy_to(out, out_bytes));
        COHORT_TRY(r.copy_to(info, sizeof *info, out_bytes));
        COHORT_TRY(r.copy_to(aliased, kColumns, out_bytes + sizeof *info));
        COHORT_TRY(s.copy_to(stat, stat_bytes));
        return m.copy_to(max, max_bytes);
    });
}

int epik_amd_cohort_edgemodel_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                   const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t num_terms,
                                   uint32_t num_permutations, uint64_t seed, epik_amd_edgemodel *out, epik_amd_edgemodel_info *info,
                                   double *stat, double *max, uint8_t *aliased)
{
    return epik_amd_cohort_edgemodel_strata_host(mass, num_samples, num_branches, first, kind, labels, values, num_terms, num_permutations,
                                                 seed, out, info, stat, max, aliased, nullptr);
}

int epik_amd_cohort_edgemodel_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                          const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t num_terms,
                                          uint32_t num_permutations, uint64_t seed, epik_amd_edgemodel *out,
                                          epik_amd_edgemodel_info *info, double *stat, double *max, uint8_t *aliased,
                                          const uint32_t *strata)
{
    return guarded("cohort_edgemodel_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(terms_valid(num_terms));
        COHORT_TRY(check_present(mass, first, kind, labels, values, out, info, aliased));
        std::string err;
        return rule_result(edgemodel_records(mass, num_samples, num_branches, first, kind, labels, values, num_terms, num_permutations, seed,
                                             out, info, stat, max, aliased, err, strata),
                           err);
    });
}

}  // extern "C"
