// squash_place.hip -- squash clustering (Matsen & Evans 2013) of a cohort's samples on the device:
// epik_amd_cohort_squash_device / _squash / _squash_host (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h beside the KR rule (DESIGN.md 3.9;
// epik_amd/host/cohort.cpp: squash_merges is the same rule on the CPU).  A merged cluster is a mass distribution of its
// own -- the weighted average of the planes of its two parts -- and every distance to it is again the KR rule's strictly
// sequential sum over the branches, so the records are the same bits here, on the host and in the tests' numpy.  Nothing
// is fused (__dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn; the file is built with -ffp-contract=off as well).
//
// Start-up: cohort_normalise_kernel and cohort_kr_kernel (cohort_place.hip) into a matrix D[S][S] of the squash
// workspace's own, then squash_init_kernel: live[s] = T_s > 0, w[s] = 1, node[s] = s, the control block "none".
// Then three kernels a step, all S - 1 steps enqueued up front.  The kernel boundary is the only barrier between
// workgroups; every kernel reads (r, c) from the control block the step's pick left there and returns uniformly when it
// says "none", so the host never reads back inside the loop.
//
//   squash_rows_kernel   first the COMMIT of the step before: the merged planes go into column r of the planes (in the
//                        distance kernel it would race with the lanes still reading column r; here nobody reads the
//                        planes).  Then a wave a row, grid-stride: the minimum over the live c > r of D[r][c], lanes
//                        striding the row (coalesced), compared by (value, c) so that the row's first minimum wins
//                        whatever the lane order.
//   squash_pick_kernel   every workgroup reduces the S row minima by (value, r) -- S * 12 bytes out of L2, cheaper than
//                        a kernel of one workgroup and a boundary -- and so knows (r, c, dist); workgroup 0 writes the
//                        control block.  Then the averaging, shared out over the branches: C_m, B_m into a contiguous
//                        merged[2][N].
//   squash_dist_kernel   a lane a slot x: KR(m, x) with b ascending.  The planes are [b][Sp], sample fastest: a wave reads
//                        512 contiguous bytes per plane and branch.  merged[b] and half[b] are the same for every lane:
//                        staged in LDS a unit of 32 branches at a time and read back as broadcasts.  The next unit --
//                        32 branches of column x and the lane's share of the uniform values, all into registers -- is
//                        requested before the dependent add chain of this one: 32 branches of chain are
//                        about the latency of an L2 hit (8 were not: 97 ns a branch measured, the loads exposed).  A
//                        workgroup is one wave, so the two barriers a unit cost nothing.  The lanes of r and c
//                        give len_a and len_b (the planes of r are still those of before the merge: the commit is the
//                        next kernel's), every other live lane D[r][x] = D[x][r].  The lane of r writes the rest of the
//                        record and w[r], node[r], live[c], which no other lane of this kernel reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kNone = EPIK_AMD_SQUASH_NONE;
constexpr uint32_t kUnit = 32;        // branches of column x in flight ahead of the add chain: about an L2 latency of work
constexpr uint64_t kRowBlocks = 1024;
constexpr uint64_t kPickBlocks = 256;

static_assert(sizeof(epik_amd_squash_merge) == 32);

struct SquashControl {
    double dist;
    uint32_t have, r, c, pad;
};

// the workspace, one allocation: what the kernels take
struct SquashSpace {
    double *D;          // [S][S]
    double *merged;     // C_m[N] | B_m[N]
    double *row_val;    // [S]: the minimum of row r over the live c > r
    SquashControl *ctl;
    uint32_t *row_col;  // [S]: its column, kNone: none
    uint32_t *live, *w, *node;  // [S] each
};

// the bytes of the workspace for S samples and N branches; with `base`, where its parts lie
size_t squash_space(void *base, uint32_t S, uint32_t N, SquashSpace *sp)
{
    Carver c(base);
    const SquashSpace parts{.D = c.take<double>((size_t)S * S),
                            .merged = c.take<double>(2 * (size_t)N),
                            .row_val = c.take<double>(S),
                            .ctl = c.take<SquashControl>(1),
                            .row_col = c.take<uint32_t>(S),
                            .live = c.take<uint32_t>(S),
                            .w = c.take<uint32_t>(S),
                            .node = c.take<uint32_t>(S)};
    if (sp) *sp = parts;
    return c.bytes();
}

__global__ __launch_bounds__(kBlock) void squash_init_kernel(const uint64_t *__restrict__ total, uint32_t num_samples,
                                                             uint32_t *__restrict__ live, uint32_t *__restrict__ w,
                                                             uint32_t *__restrict__ node, SquashControl *__restrict__ ctl,
                                                             uint32_t *__restrict__ num_merges)
{
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < num_samples; s += gridDim.x * kBlock)
        live[s] = total[s] != 0 ? 1u : 0u, w[s] = 1u, node[s] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *ctl = SquashControl{0.0, 0u, kNone, kNone, 0u};
        *num_merges = 0;
    }
}

// whether (v, k) comes before (best_v, best_k): the smaller value, then the smaller index; kNone is no candidate
__device__ inline bool comes_first(double v, uint32_t k, bool have, double best_v, uint32_t best_k, bool best_have)
{
    return have && (!best_have || v < best_v || (v == best_v && k < best_k));
}

__global__ __launch_bounds__(kBlock) void squash_rows_kernel(double *__restrict__ planes, uint32_t num_branches, uint32_t padded,
                                                             const double *__restrict__ merged,
                                                             const SquashControl *__restrict__ ctl, const double *__restrict__ D,
                                                             const uint32_t *__restrict__ live, uint32_t num_samples,
                                                             double *__restrict__ row_val, uint32_t *__restrict__ row_col)
{
    if (ctl->have) {  // the commit of the step before: column r takes the merged planes
        const uint32_t r = ctl->r;
        double *C = planes, *B = planes + (uint64_t)num_branches * padded;
        for (uint32_t b = blockIdx.x * kBlock + threadIdx.x; b < num_branches; b += gridDim.x * kBlock) {
            C[(uint64_t)b * padded + r] = merged[b];
            B[(uint64_t)b * padded + r] = merged[num_branches + b];
        }
    }
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (uint32_t r = blockIdx.x * kBlockWaves + wave; r < num_samples; r += gridDim.x * kBlockWaves) {
        double val = 0.0;
        uint32_t col = kNone;
        if (live[r]) {
            const double *row = D + (uint64_t)r * num_samples;
            for (uint32_t c = r + 1 + lane; c < num_samples; c += kWave) {  // (ascending in a lane: strict < keeps the first)
                if (!live[c]) continue;
                const double v = row[c];
                if (col == kNone || v < val) val = v, col = c;
            }
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const double ov = __shfl_down(val, d);
            const uint32_t oc = __shfl_down(col, d);
            if (comes_first(ov, oc, oc != kNone, val, col, col != kNone)) val = ov, col = oc;
        }
        if (lane == 0) row_val[r] = val, row_col[r] = col;
    }
}

__global__ __launch_bounds__(kBlock) void squash_pick_kernel(const double *__restrict__ planes, uint32_t num_branches, uint32_t padded,
                                                             uint32_t num_samples, const double *__restrict__ row_val,
                                                             const uint32_t *__restrict__ row_col, const uint32_t *__restrict__ w,
                                                             double *__restrict__ merged, SquashControl *__restrict__ ctl)
{
    __shared__ double wave_val[kBlockWaves];
    __shared__ uint32_t wave_row[kBlockWaves], wave_col[kBlockWaves];
    double val = 0.0;
    uint32_t row = kNone, col = kNone;
    for (uint32_t r = threadIdx.x; r < num_samples; r += kBlock) {  // (ascending in a lane: strict < keeps the first)
        const uint32_t c = row_col[r];
        if (c == kNone) continue;
        const double v = row_val[r];
        if (row == kNone || v < val) val = v, row = r, col = c;
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const double ov = __shfl_down(val, d);
        const uint32_t orow = __shfl_down(row, d), oc = __shfl_down(col, d);
        if (comes_first(ov, orow, orow != kNone, val, row, row != kNone)) val = ov, row = orow, col = oc;
    }
    if (threadIdx.x % kWave == 0) wave_val[threadIdx.x / kWave] = val, wave_row[threadIdx.x / kWave] = row, wave_col[threadIdx.x / kWave] = col;
    __syncthreads();
    val = wave_val[0], row = wave_row[0], col = wave_col[0];
#pragma unroll
    for (uint32_t k = 1; k < kBlockWaves; ++k)
        if (comes_first(wave_val[k], wave_row[k], wave_row[k] != kNone, val, row, row != kNone))
            val = wave_val[k], row = wave_row[k], col = wave_col[k];
    // (the same in every lane of every workgroup from here)
    if (row == kNone) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *ctl = SquashControl{0.0, 0u, kNone, kNone, 0u};
        return;
    }
    const double wr = (double)w[row], wc = (double)w[col], W = (double)(w[row] + w[col]);
    const double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    for (uint32_t b = blockIdx.x * kBlock + threadIdx.x; b < num_branches; b += gridDim.x * kBlock) {
        const uint64_t at = (uint64_t)b * padded;
        merged[b] = __ddiv_rn(__dadd_rn(__dmul_rn(wr, C[at + row]), __dmul_rn(wc, C[at + col])), W);
        merged[num_branches + b] = __ddiv_rn(__dadd_rn(__dmul_rn(wr, B[at + row]), __dmul_rn(wc, B[at + col])), W);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *ctl = SquashControl{val, 1u, row, col, 0u};
}

__device__ inline double kr_step(double acc, double h, double cm, double bm, double cx, double bx)
{
    return __dadd_rn(acc, __dmul_rn(h, __dadd_rn(fabs(__dsub_rn(cm, cx)), fabs(__dsub_rn(bm, bx)))));
}

__global__ __launch_bounds__(kWave) void squash_dist_kernel(const double *__restrict__ planes, uint32_t num_branches, uint32_t padded,
                                                            const double *__restrict__ half, const double *__restrict__ merged,
                                                            const SquashControl *__restrict__ ctl, double *__restrict__ D,
                                                            uint32_t *live, uint32_t *w, uint32_t *node, uint32_t num_samples,
                                                            uint32_t step, epik_amd_squash_merge *__restrict__ merges,
                                                            uint32_t *__restrict__ num_merges)
{
    __shared__ double s_cm[kUnit], s_bm[kUnit], s_half[kUnit];  // C_m, B_m, half of the unit at hand
    if (!ctl->have) {  // (uniform: the clustering is over; the record is written by rule)
        if (blockIdx.x == 0 && threadIdx.x == 0) merges[step] = epik_amd_squash_merge{kNone, kNone, 0.0, 0.0, 0.0};
        return;
    }
    const uint32_t r = ctl->r, c = ctl->c, lane = threadIdx.x;
    const double *Cm = merged, *Bm = merged + num_branches;
    const uint32_t full = num_branches / kUnit * kUnit;
    // a workgroup is one wave of 64 slots; every lane walks the branches (the barriers), a lane without a slot to
    // compute walks the last sample's column and writes nothing
    for (uint32_t x0 = blockIdx.x * kWave; x0 < num_samples; x0 += gridDim.x * kWave) {
        const uint32_t slot = x0 + lane, x = slot < num_samples ? slot : num_samples - 1;
        const bool mine = slot < num_samples && (x == r || x == c || live[x]);  // (live[c] is written below by the lane of r only)
        const double *Cx = planes + x, *Bx = planes + (uint64_t)num_branches * padded + x;
        const uint32_t mine_of_unit = lane % kUnit;  // the branch of a unit whose uniform values this lane fetches
        double acc = 0.0;
        // two sets of registers, each a unit: its 32 branches of column x and this lane's share of the uniform values.
        // One is computed on while the other is in flight; they swap roles by name, never by copy (a copy is a use: the
        // compiler schedules it early and waits for the loads there).
        struct Unit {
            double c[kUnit], b[kUnit], cm, bm, hf;
        } u0 = {}, u1 = {};
        const auto fetch = [&](Unit &u, uint32_t b0) {
            u.cm = Cm[b0 + mine_of_unit], u.bm = Bm[b0 + mine_of_unit], u.hf = half[b0 + mine_of_unit];
            const double *pc = Cx + (uint64_t)b0 * padded, *pb = Bx + (uint64_t)b0 * padded;  // (one add an address, no multiply)
#pragma unroll
            for (uint32_t k = 0; k < kUnit; ++k, pc += padded, pb += padded) u.c[k] = *pc, u.b[k] = *pb;
        };
        const auto unit = [&](const Unit &cur, Unit &nxt, uint32_t b0, bool keep) {
            // this unit's uniform values, asked for a unit ago, go to LDS (the reads of the unit before are done: one wave;
            // every lane stores, two to a value: under a condition the compiler moves the loads down to the stores)
            __syncthreads();
            s_cm[mine_of_unit] = cur.cm, s_bm[mine_of_unit] = cur.bm, s_half[mine_of_unit] = cur.hf;
            __syncthreads();
            // the next unit is asked for before the dependent add chain of this one (the last unit asks for itself again)
            fetch(nxt, b0 + kUnit < full ? b0 + kUnit : b0);
            double sum = acc;
#pragma unroll
            for (uint32_t k = 0; k < kUnit; ++k)  // ascending, one branch after the other: the rule's order
                sum = kr_step(sum, s_half[k], s_cm[k], s_bm[k], cur.c[k], cur.b[k]);
            acc = keep ? sum : acc;
        };
        if (full) fetch(u0, 0);
        // two units a round and no branch between them: a set used only under a condition has its loads moved down
        // into that condition, next to their use.  With an odd number of units the last round walks its unit twice
        // and keeps the first sum.
        for (uint32_t b0 = 0; b0 < full; b0 += 2 * kUnit) {
            const bool second = b0 + kUnit < full;
            unit(u0, u1, b0, true);
            unit(u1, u0, second ? b0 + kUnit : b0, second);
        }
        for (uint32_t b = full; b < num_branches; ++b)  // the last N % kUnit branches: uniform loads
            acc = kr_step(acc, half[b], Cm[b], Bm[b], Cx[(uint64_t)b * padded], Bx[(uint64_t)b * padded]);
        if (!mine) continue;
        if (x == r) {
            merges[step].a = node[r], merges[step].b = node[c], merges[step].dist = ctl->dist, merges[step].len_a = acc;
            node[r] = num_samples + step, w[r] += w[c], live[c] = 0;
            *num_merges = step + 1;
        } else if (x == c) {
            merges[step].len_b = acc;
        } else {
            D[(uint64_t)r * num_samples + x] = acc;
            D[(uint64_t)x * num_samples + r] = acc;
        }
    }
}

int squash_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_merges,
                       void *d_num_merges, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    const uint32_t N = cohort->num_branches, S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    COHORT_TRY(check_present(branch_length, d_num_merges));
    if (S > 1) COHORT_TRY(check_present(d_merges));
    HIP_TRY(hipSetDevice(cohort->device));
    // (one size a cohort: allocated by the first call and never freed by a later one, so the device need not be drained yet)
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceSquash, squash_space(nullptr, S, N, nullptr)));
    SquashSpace sp;
    squash_space(cohort->space[kSpaceSquash].d, S, N, &sp);
    // the checks of the tree and the lengths, the planes and D = the KR matrix; it will be overwritten
    COHORT_TRY(cohort_kr_enqueue(cohort, tree, branch_length, sp.D, stream));
    auto *merges = static_cast<epik_amd_squash_merge *>(d_merges);
    auto *num_merges = static_cast<uint32_t *>(d_num_merges);
    hipLaunchKernelGGL(squash_init_kernel, cohort_grid_per(cohort, S, kBlock, kRowBlocks), dim3(kBlock), 0, stream, cohort->d_total, S, sp.live, sp.w,
                       sp.node, sp.ctl, num_merges);
    HIP_TRY(hipGetLastError());
    const dim3 row_grid = cohort_grid_per(cohort, std::max(S, (N + kBlock - 1) / kBlock * kBlockWaves), kBlockWaves, kRowBlocks);
    const dim3 pick_grid = cohort_grid_per(cohort, N, kBlock, kPickBlocks), dist_grid = cohort_grid_per(cohort, S, kWave, kRowBlocks);
    for (uint32_t step = 0; step + 1 < S; ++step) {
        hipLaunchKernelGGL(squash_rows_kernel, row_grid, dim3(kBlock), 0, stream, cohort->d_planes, N, padded, sp.merged, sp.ctl, sp.D,
                           sp.live, S, sp.row_val, sp.row_col);
        hipLaunchKernelGGL(squash_pick_kernel, pick_grid, dim3(kBlock), 0, stream, cohort->d_planes, N, padded, S, sp.row_val,
                           sp.row_col, sp.w, sp.merged, sp.ctl);
        hipLaunchKernelGGL(squash_dist_kernel, dist_grid, dim3(kWave), 0, stream, cohort->d_planes, N, padded, cohort->d_half,
                           sp.merged, sp.ctl, sp.D, sp.live, sp.w, sp.node, S, step, merges, num_merges);
        HIP_TRY(hipGetLastError());
    }
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_squash_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                  void *d_merges, void *d_num_merges, void *stream)
{
    return guarded("cohort_squash_device", [&]() -> int {
        return squash_device_impl(cohort, tree, branch_length, d_merges, d_num_merges, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_squash(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                           epik_amd_squash_merge *merges, uint32_t *num_merges)
{
    return guarded("cohort_squash", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        const size_t records = cohort->num_samples - 1, bytes = records * sizeof(epik_amd_squash_merge);
        COHORT_TRY(check_present(num_merges));
        if (records) COHORT_TRY(check_present(merges));
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult m;
        COHORT_TRY(m.alloc(bytes + sizeof(uint32_t)));  // the records, then the count
        COHORT_TRY(squash_device_impl(cohort, tree, branch_length, m.d, m.at(bytes), nullptr));
        if (records) COHORT_TRY(m.copy_to(merges, bytes));
        return m.copy_to(num_merges, sizeof(uint32_t), bytes);
    });
}

int epik_amd_cohort_squash_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, epik_amd_squash_merge *merges, uint32_t *num_merges)
{
    return guarded("cohort_squash_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, num_merges));
        if (num_samples > 1) COHORT_TRY(check_present(merges));
        std::string err;
        return rule_result(squash_merges(mass, num_samples, num_branches, first, branch_length, merges, num_merges, err), err);
    });
}

}  // extern "C"
