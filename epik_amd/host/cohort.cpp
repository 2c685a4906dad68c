#include "cohort.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <stdexcept>
#include <tuple>

namespace epik_amd {

namespace {

inline uint64_t cohort_q(double lwr) { return (uint64_t)std::llrint(lwr * (double)(1u << EPIK_AMD_PROFILE_LWR_BITS)); }

}  // namespace

void sample_cohort::add_rows(const epik_amd_placement* rows, const uint32_t* n_rows, const uint32_t* kmer_counts,
                             const uint32_t* weights, const uint32_t* samples, uint64_t n, uint32_t keep)
{
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t s = samples[i];
        if (s >= num_samples) {
            ++bad_samples;
            continue;
        }
        // the profile's rule (profile.cpp: add_read), on row s
        uint64_t* m = mass.data() + (size_t)s * num_branches;
        uint64_t* b = best.data() + (size_t)s * num_branches;
        auto& t = totals[s];
        const uint32_t w = weights ? weights[i] : 1u;
        const uint32_t nr = n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW || n_rows[i] <= keep ? n_rows[i] : keep;
        if (nr == EPIK_AMD_ROWS_COUNTS_TOO_NARROW) {
            t.too_narrow += w;
        } else if (nr == 0) {
            t.too_short += w;
        } else if (kmer_counts[i * keep] == 0) {
            t.no_hit += w;
        } else {
            t.placed += w;
            for (uint32_t j = 0; j < nr; ++j) {
                const auto& r = rows[i * keep + j];
                if (r.branch >= num_branches) {
                    ++t.bad_rows;
                    continue;
                }
                m[r.branch] += (uint64_t)w * cohort_q(r.lwr);
                if (j == 0) b[r.branch] += w;
            }
        }
    }
}

void sample_cohort::add_cells(const uint64_t* other_mass, const uint64_t* other_best, const epik_amd_profile_totals* other_totals)
{
    const size_t cells = (size_t)num_samples * num_branches;
    if (other_mass)
        for (size_t c = 0; c < cells; ++c) mass[c] += other_mass[c];
    if (other_best)
        for (size_t c = 0; c < cells; ++c) best[c] += other_best[c];
    if (other_totals)
        for (uint32_t s = 0; s < num_samples; ++s) {
            totals[s].placed += other_totals[s].placed, totals[s].no_hit += other_totals[s].no_hit;
            totals[s].too_short += other_totals[s].too_short, totals[s].too_narrow += other_totals[s].too_narrow;
            totals[s].bad_rows += other_totals[s].bad_rows;
        }
}

void sample_cohort::merge(const sample_cohort& other)
{
    if (other.num_samples != num_samples || other.num_branches != num_branches)
        throw std::runtime_error("cohorts of different shapes");
    add_cells(other.mass.data(), other.best.data(), other.totals.data());
    bad_samples += other.bad_samples;
}

namespace {

// what both the distance matrix and the clustering start from: first[] and the lengths checked, half[b] = 0.5 * bl[b],
// T_s, and C[s][b], B[s][b] -- one conversion each and one division; T_s == 0 leaves the row unused.  Edge PCA takes no
// lengths: branch_length may be null, and half stays zero
struct kr_planes {
    std::vector<double> C, B, half;
    std::vector<uint64_t> total;
};

int make_planes(const uint64_t* mass, size_t S, size_t N, const uint32_t* first, const double* branch_length, kr_planes& p,
                std::string& err)
{
    for (size_t b = 0; b < N; ++b) {
        if (first[b] > b) {
            err = "branch " + std::to_string(b) + ": first[b] = " + std::to_string(first[b]) + " is above the branch";
            return EPIK_AMD_ERR_INVALID;
        }
        if (branch_length && (!(branch_length[b] >= 0.0) || !std::isfinite(branch_length[b]))) {
            err = "branch " + std::to_string(b) + ": the branch length is negative or not finite";
            return EPIK_AMD_ERR_INVALID;
        }
    }
    p.C.assign(S * N, 0.0), p.B.assign(S * N, 0.0), p.half.assign(N, 0.0), p.total.assign(S, 0);
    std::vector<uint64_t> prefix(N + 1);
    for (size_t b = 0; branch_length && b < N; ++b) p.half[b] = 0.5 * branch_length[b];
    for (size_t s = 0; s < S; ++s) {
        const uint64_t* m = mass + s * N;
        prefix[0] = 0;
        for (size_t b = 0; b < N; ++b) prefix[b + 1] = prefix[b] + m[b];
        p.total[s] = prefix[N];
        if (p.total[s] == 0) continue;
        const double T = (double)p.total[s];
        for (size_t b = 0; b < N; ++b) {
            const uint64_t clade = prefix[b + 1] - prefix[first[b]], below = clade - m[b];
            p.C[s * N + b] = (double)clade / T;
            p.B[s * N + b] = (double)below / T;
        }
    }
    return EPIK_AMD_OK;
}

// the rule's sequential sum over two pairs of planes
inline double kr_of(const double* cx, const double* bx, const double* cy, const double* by, const double* half, size_t N)
{
    double acc = 0.0;
    for (size_t b = 0; b < N; ++b) acc = acc + half[b] * (std::fabs(cx[b] - cy[b]) + std::fabs(bx[b] - by[b]));
    return acc;
}

}  // namespace

int kr_matrix(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
              const double* branch_length, double* out, std::string& err)
{
    const size_t S = num_samples, N = num_branches;
    kr_planes p;
    if (const int rc = make_planes(mass, S, N, first, branch_length, p, err); rc != EPIK_AMD_OK) return rc;
    for (size_t s = 0; s < S; ++s) {
        out[s * S + s] = 0.0;
        for (size_t t = s + 1; t < S; ++t) {
            double acc = -1.0;
            if (p.total[s] != 0 && p.total[t] != 0)
                acc = kr_of(&p.C[s * N], &p.B[s * N], &p.C[t * N], &p.B[t * N], p.half.data(), N);
            out[s * S + t] = out[t * S + s] = acc;
        }
    }
    return EPIK_AMD_OK;
}

namespace {

// one half-branch of one pair: its terms of the UniFrac rule's tn_b and td_b
template <uint32_t Metric>
inline void unifrac_half(double x, double y, double& tn, double& td)
{
    if (Metric == EPIK_AMD_DISTANCE_UNWEIGHTED) {
        const bool px = x > 0.0, py = y > 0.0;
        tn = px != py ? 1.0 : 0.0;
        td = px || py ? 1.0 : 0.0;
    } else if (Metric == EPIK_AMD_DISTANCE_WEIGHTED) {
        tn = std::fabs(x - y);
        td = x + y;
    } else {
        const double sum = x + y;
        td = std::sqrt(sum);
        tn = sum > 0.0 ? td * (std::fabs(x - y) / sum) : 0.0;
    }
}

// the rule's two sequential sums over two pairs of planes, then den == 0 and the one division
template <uint32_t Metric>
double unifrac_of(const double* cx, const double* bx, const double* cy, const double* by, const double* half, size_t N)
{
    double num = 0.0, den = 0.0;
    for (size_t b = 0; b < N; ++b) {
        double cn, cd, bn, bd;
        unifrac_half<Metric>(cx[b], cy[b], cn, cd);
        unifrac_half<Metric>(bx[b], by[b], bn, bd);
        num = num + half[b] * (cn + bn);
        den = den + half[b] * (cd + bd);
    }
    return den == 0.0 ? 0.0 : num / den;
}

}  // namespace

int unifrac_matrix(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                   const double* branch_length, uint32_t metric, double* out, std::string& err)
{
    if (metric < EPIK_AMD_DISTANCE_UNWEIGHTED || metric > EPIK_AMD_DISTANCE_GENERALIZED) {
        err = "metric = " + std::to_string(metric) + " is no UniFrac distance (1 unweighted, 2 weighted, 3 generalized)";
        return EPIK_AMD_ERR_INVALID;
    }
    const size_t S = num_samples, N = num_branches;
    kr_planes p;
    if (const int rc = make_planes(mass, S, N, first, branch_length, p, err); rc != EPIK_AMD_OK) return rc;
    const auto of = metric == EPIK_AMD_DISTANCE_UNWEIGHTED ? unifrac_of<EPIK_AMD_DISTANCE_UNWEIGHTED>
                    : metric == EPIK_AMD_DISTANCE_WEIGHTED ? unifrac_of<EPIK_AMD_DISTANCE_WEIGHTED>
                                                           : unifrac_of<EPIK_AMD_DISTANCE_GENERALIZED>;
    for (size_t s = 0; s < S; ++s) {
        out[s * S + s] = 0.0;
        for (size_t t = s + 1; t < S; ++t) {
            double d = -1.0;
            if (p.total[s] != 0 && p.total[t] != 0) d = of(&p.C[s * N], &p.B[s * N], &p.C[t * N], &p.B[t * N], p.half.data(), N);
            out[s * S + t] = out[t * S + s] = d;
        }
    }
    return EPIK_AMD_OK;
}

int distance_matrix(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                    const double* branch_length, uint32_t metric, double* out, std::string& err)
{
    if (metric == EPIK_AMD_DISTANCE_KR) return kr_matrix(mass, num_samples, num_branches, first, branch_length, out, err);
    if (metric > EPIK_AMD_DISTANCE_GENERALIZED) {
        err = "metric = " + std::to_string(metric) + " is no distance (0 kr, 1 unweighted, 2 weighted, 3 generalized)";
        return EPIK_AMD_ERR_INVALID;
    }
    return unifrac_matrix(mass, num_samples, num_branches, first, branch_length, metric, out, err);
}

int squash_merges(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                  const double* branch_length, epik_amd_squash_merge* merges, uint32_t* num_merges, std::string& err)
{
    const size_t S = num_samples, N = num_branches;
    kr_planes p;
    if (const int rc = make_planes(mass, S, N, first, branch_length, p, err); rc != EPIK_AMD_OK) return rc;
    std::vector<char> live(S);
    std::vector<uint32_t> w(S, 1), node(S);
    std::vector<double> D(S * S, 0.0), Cm(N), Bm(N);
    for (size_t s = 0; s < S; ++s) live[s] = p.total[s] != 0, node[s] = (uint32_t)s;
    for (size_t r = 0; r < S; ++r)
        for (size_t c = r + 1; c < S; ++c)
            if (live[r] && live[c])
                D[r * S + c] = D[c * S + r] = kr_of(&p.C[r * N], &p.B[r * N], &p.C[c * N], &p.B[c * N], p.half.data(), N);
    uint32_t t = 0;
    for (;; ++t) {
        // the first pair, in row-major order, with the smallest distance
        size_t r = S, c = S;
        for (size_t i = 0; i < S; ++i)
            for (size_t j = i + 1; live[i] && j < S; ++j)
                if (live[j] && (r == S || D[i * S + j] < D[r * S + c])) r = i, c = j;
        if (r == S) break;
        double *cr = &p.C[r * N], *br = &p.B[r * N];
        const double *cc = &p.C[c * N], *bc = &p.B[c * N];
        const double wr = (double)w[r], wc = (double)w[c], W = (double)(w[r] + w[c]);
        for (size_t b = 0; b < N; ++b) {
            Cm[b] = (wr * cr[b] + wc * cc[b]) / W;
            Bm[b] = (wr * br[b] + wc * bc[b]) / W;
        }
        merges[t] = epik_amd_squash_merge{node[r], node[c], D[r * S + c], kr_of(Cm.data(), Bm.data(), cr, br, p.half.data(), N),
                                          kr_of(Cm.data(), Bm.data(), cc, bc, p.half.data(), N)};
        for (size_t b = 0; b < N; ++b) cr[b] = Cm[b], br[b] = Bm[b];
        w[r] += w[c], node[r] = (uint32_t)(S + t), live[c] = 0;
        for (size_t x = 0; x < S; ++x)
            if (live[x] && x != r)
                D[r * S + x] = D[x * S + r] = kr_of(cr, br, &p.C[x * N], &p.B[x * N], p.half.data(), N);
    }
    *num_merges = t;
    for (size_t k = t; k + 1 < S; ++k) merges[k] = epik_amd_squash_merge{EPIK_AMD_SQUASH_NONE, EPIK_AMD_SQUASH_NONE, 0.0, 0.0, 0.0};
    return EPIK_AMD_OK;
}

namespace {

// The Jacobi paragraph of the edge-PCA rule on A[L][L] (symmetric) and V[L][L] (the identity on entry): cyclic, round-robin,
// the rotations of a round applied together.  The principal coordinates take it as it is.
void jacobi_sweeps(std::vector<double>& A, std::vector<double>& V, size_t L, double tol, uint32_t& sweeps, uint32_t& converged)
{
    std::vector<double> A1(L * L), V1(L * L);
    const size_t m = L + L % 2;
    std::vector<double> cs(L), sn(L);
    std::vector<size_t> partner(L);
    std::vector<char> rot(L);
    sweeps = 0, converged = 0;
    while (sweeps < EPIK_AMD_JACOBI_MAX_SWEEPS && !converged) {
        ++sweeps;
        size_t rotated = 0;
        for (size_t r = 0; r + 1 < m; ++r) {
            std::fill(rot.begin(), rot.end(), 0);
            size_t in_round = 0;
            for (size_t i = 0; i < m / 2; ++i) {
                const size_t x = i ? (r + i) % (m - 1) : r, y = i ? (r + m - 1 - i) % (m - 1) : m - 1;
                const size_t pp = std::min(x, y), q = std::max(x, y);
                if (q >= L) continue;
                const double apq = A[pp * L + q];
                if (!(std::fabs(apq) > tol)) continue;
                const double theta = (A[q * L + q] - A[pp * L + pp]) / (2.0 * apq);
                double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                rot[pp] = rot[q] = 1, cs[pp] = cs[q] = c, sn[pp] = s, sn[q] = -s, partner[pp] = q, partner[q] = pp;
                ++in_round;
            }
            if (!in_round) continue;
            rotated += in_round;
            for (size_t i = 0; i < L; ++i)  // the column phase, on the full matrix
                for (size_t j = 0; j < L; ++j) {
                    const bool turn = rot[j];
                    A1[i * L + j] = turn ? cs[j] * A[i * L + j] - sn[j] * A[i * L + partner[j]] : A[i * L + j];
                    V1[i * L + j] = turn ? cs[j] * V[i * L + j] - sn[j] * V[i * L + partner[j]] : V[i * L + j];
                }
            V.swap(V1);
            for (size_t i = 0; i < L; ++i)  // the row phase on i <= j, mirrored
                for (size_t j = i; j < L; ++j) {
                    const double v = rot[i] ? cs[i] * A1[i * L + j] - sn[i] * A1[partner[i] * L + j] : A1[i * L + j];
                    A[i * L + j] = A[j * L + i] = v;
                }
            for (size_t j = 0; j < L; ++j)
                if (rot[j]) A[j * L + partner[j]] = 0.0;
        }
        converged = rotated == 0;
    }
}

}  // namespace

int epca_components(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                    uint32_t num_components, double* mu, double* proj, double* edge, epik_amd_epca_info* info, std::string& err)
{
    const size_t S = num_samples, N = num_branches, K = num_components;
    if (K < 1 || K > EPIK_AMD_EPCA_MAX_COMPONENTS) {
        err = "num_components = " + std::to_string(K) + " is outside [1, 64]";
        return EPIK_AMD_ERR_INVALID;
    }
    kr_planes p;
    if (const int rc = make_planes(mass, S, N, first, nullptr, p, err); rc != EPIK_AMD_OK) return rc;
    std::vector<size_t> used;
    for (size_t s = 0; s < S; ++s)
        if (p.total[s] != 0) used.push_back(s);
    const size_t L = used.size(), Kc = std::min(K, L);
    // the centred imbalances Y[j][b]
    std::vector<double> Y(L * N, 0.0);
    for (size_t b = 0; b < N; ++b) {
        const bool inner = first[b] < b;
        double acc = 0.0;
        for (size_t j = 0; j < L; ++j) {
            const double x = inner ? (p.B[used[j] * N + b] + p.C[used[j] * N + b]) - 1.0 : 0.0;
            Y[j * N + b] = x;
            acc = acc + x;
        }
        const double mean = L ? acc / (double)L : 0.0;
        for (size_t j = 0; j < L; ++j) Y[j * N + b] = Y[j * N + b] - mean;
    }
    // the Gram matrix, its scale and trace
    std::vector<double> A(L * L, 0.0), V(L * L, 0.0);
    for (size_t i = 0; i < L; ++i)
        for (size_t j = i; j < L; ++j) {
            const double *yi = &Y[i * N], *yj = &Y[j * N];
            double acc = 0.0;
            for (size_t b = 0; b < N; ++b) acc = acc + yi[b] * yj[b];
            A[i * L + j] = A[j * L + i] = acc;
        }
    double scale = 0.0, trace = 0.0;
    for (size_t j = 0; j < L; ++j) {
        if (A[j * L + j] > scale) scale = A[j * L + j];
        trace = trace + A[j * L + j];
        V[j * L + j] = 1.0;
    }
    const double tol = std::ldexp(1.0, -52) * scale;
    uint32_t sweeps = 0, converged = 0;
    jacobi_sweeps(A, V, L, tol, sweeps, converged);
    // the components: by (mu descending, j ascending)
    std::vector<size_t> column(Kc);
    for (size_t j = 0; j < L; ++j) {
        size_t rank = 0;
        for (size_t i = 0; i < L; ++i)
            rank += A[i * L + i] > A[j * L + j] || (A[i * L + i] == A[j * L + j] && i < j) ? 1 : 0;
        if (rank < Kc) column[rank] = j;
    }
    std::fill(mu, mu + K, 0.0), std::fill(proj, proj + S * K, 0.0), std::fill(edge, edge + K * N, 0.0);
    const double floor_mu = std::ldexp(1.0, -40) * scale;
    std::vector<double> raw(N);
    for (size_t k = 0; k < Kc; ++k) {
        const size_t jk = column[k];
        mu[k] = A[jk * L + jk];
        if (!(mu[k] > floor_mu)) continue;
        const double r = std::sqrt(mu[k]);
        size_t at = 0;
        for (size_t b = 0; b < N; ++b) {
            double acc = 0.0;
            for (size_t j = 0; j < L; ++j) acc = acc + V[j * L + jk] * Y[j * N + b];
            raw[b] = acc;
            if (std::fabs(acc) > std::fabs(raw[at])) at = b;
        }
        const double sign = raw[at] < 0.0 ? -1.0 : 1.0;
        for (size_t b = 0; b < N; ++b) edge[k * N + b] = sign * (raw[b] / r);
        for (size_t j = 0; j < L; ++j) proj[used[j] * K + k] = sign * (V[j * L + jk] * r);
    }
    *info = epik_amd_epca_info{(uint32_t)L, (uint32_t)Kc, sweeps, converged, trace, scale};
    return EPIK_AMD_OK;
}

int kmeans_clusters(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                    const double* branch_length, uint32_t num_clusters, uint32_t max_iterations, epik_amd_kmeans_sample* samples,
                    epik_amd_kmeans_cluster* clusters, double* centroids, epik_amd_kmeans_info* info, std::string& err)
{
    const size_t S = num_samples, N = num_branches, K = num_clusters;
    if (K < 1 || K > EPIK_AMD_KMEANS_MAX_CLUSTERS) {
        err = "num_clusters = " + std::to_string(K) + " is outside [1, 64]";
        return EPIK_AMD_ERR_INVALID;
    }
    if (max_iterations < 1 || max_iterations > EPIK_AMD_KMEANS_MAX_ITERATIONS) {
        err = "max_iterations = " + std::to_string(max_iterations) + " is outside [1, 1000]";
        return EPIK_AMD_ERR_INVALID;
    }
    kr_planes p;
    if (const int rc = make_planes(mass, S, N, first, branch_length, p, err); rc != EPIK_AMD_OK) return rc;
    std::vector<size_t> used;
    for (size_t s = 0; s < S; ++s)
        if (p.total[s] != 0) used.push_back(s);
    const size_t L = used.size(), Kc = std::min(K, L);
    const double* half = p.half.data();
    for (size_t s = 0; s < S; ++s) samples[s] = epik_amd_kmeans_sample{EPIK_AMD_KMEANS_NONE, 0u, -1.0};
    for (size_t k = 0; k < K; ++k) clusters[k] = epik_amd_kmeans_cluster{0u, EPIK_AMD_KMEANS_NONE, 0.0, 0.0};
    std::fill(centroids, centroids + K * N, 0.0);
    *info = epik_amd_kmeans_info{0u, 0u, 0u, 1u};
    if (L == 0) return EPIK_AMD_OK;
    const auto plane_c = [&](size_t j) { return &p.C[used[j] * N]; };
    const auto plane_b = [&](size_t j) { return &p.B[used[j] * N]; };
    // the average of the planes of `members` (ascending j) into cc[N], cb[N]
    const auto average = [&](const std::vector<size_t>& members, double* cc, double* cb) {
        const double size = (double)members.size();
        for (size_t b = 0; b < N; ++b) {
            double acc_c = 0.0, acc_b = 0.0;
            for (const size_t j : members) acc_c = acc_c + plane_c(j)[b], acc_b = acc_b + plane_b(j)[b];
            cc[b] = acc_c / size, cb[b] = acc_b / size;
        }
    };
    // the seeding: the sample nearest the grand mean, then farthest first
    std::vector<double> cent_c(Kc * N), cent_b(Kc * N), mind(L);
    std::vector<size_t> everyone(L), seed(Kc);
    std::vector<char> is_centre(L, 0);
    for (size_t j = 0; j < L; ++j) everyone[j] = j;
    {
        std::vector<double> mc(N), mb(N);
        average(everyone, mc.data(), mb.data());
        size_t at = 0;
        double best = 0.0;
        for (size_t j = 0; j < L; ++j) {
            const double d = kr_of(mc.data(), mb.data(), plane_c(j), plane_b(j), half, N);
            if (j == 0 || d < best) best = d, at = j;
        }
        seed[0] = at;
    }
    for (size_t k = 0; k < Kc; ++k) {
        if (k) {
            size_t at = L;
            for (size_t j = 0; j < L; ++j)
                if (!is_centre[j] && (at == L || mind[j] > mind[at])) at = j;
            seed[k] = at;
        }
        const size_t c = seed[k];
        is_centre[c] = 1;
        std::copy(plane_c(c), plane_c(c) + N, &cent_c[k * N]);
        std::copy(plane_b(c), plane_b(c) + N, &cent_b[k * N]);
        for (size_t j = 0; j < L; ++j) {
            const double d = kr_of(&cent_c[k * N], &cent_b[k * N], plane_c(j), plane_b(j), half, N);
            mind[j] = k == 0 || d < mind[j] ? d : mind[j];
        }
    }
    // the iterations
    std::vector<size_t> assign(L, K);  // (K: none)
    std::vector<double> dist(L, 0.0);
    std::vector<std::vector<size_t>> members(Kc);
    uint32_t iterations = 0, converged = 0;
    for (;;) {
        ++iterations;
        size_t changed = 0;
        for (auto& list : members) list.clear();
        for (size_t j = 0; j < L; ++j) {
            size_t at = 0;
            double best = 0.0;
            for (size_t k = 0; k < Kc; ++k) {
                const double d = kr_of(plane_c(j), plane_b(j), &cent_c[k * N], &cent_b[k * N], half, N);
                if (k == 0 || d < best) best = d, at = k;
            }
            changed += assign[j] != at ? 1 : 0;
            assign[j] = at, dist[j] = best;
            members[at].push_back(j);
        }
        if (changed == 0) {
            converged = 1;
            break;
        }
        if (iterations == max_iterations) break;
        for (size_t k = 0; k < Kc; ++k)
            if (!members[k].empty()) average(members[k], &cent_c[k * N], &cent_b[k * N]);
    }
    for (size_t j = 0; j < L; ++j) samples[used[j]] = epik_amd_kmeans_sample{(uint32_t)assign[j], 0u, dist[j]};
    for (size_t k = 0; k < Kc; ++k) {
        double sum = 0.0, sq = 0.0;
        for (const size_t j : members[k]) sum = sum + dist[j], sq = sq + dist[j] * dist[j];
        clusters[k] = epik_amd_kmeans_cluster{(uint32_t)members[k].size(), (uint32_t)used[seed[k]], sum, sq};
        for (size_t b = 0; b < N; ++b) centroids[k * N + b] = cent_c[k * N + b] - cent_b[k * N + b];
    }
    *info = epik_amd_kmeans_info{(uint32_t)L, (uint32_t)Kc, iterations, converged};
    return EPIK_AMD_OK;
}

namespace {

constexpr size_t kDiversityBlock = EPIK_AMD_DIVERSITY_BLOCK;

// first[] and the lengths as make_planes checks them, and half[b] = 0.5 * bl[b]
int check_tree_lengths(size_t N, const uint32_t* first, const double* branch_length, std::vector<double>& half, std::string& err)
{
    half.assign(N, 0.0);
    for (size_t b = 0; b < N; ++b) {
        if (first[b] > b) {
            err = "branch " + std::to_string(b) + ": first[b] = " + std::to_string(first[b]) + " is above the branch";
            return EPIK_AMD_ERR_INVALID;
        }
        if (!(branch_length[b] >= 0.0) || !std::isfinite(branch_length[b])) {
            err = "branch " + std::to_string(b) + ": the branch length is negative or not finite";
            return EPIK_AMD_ERR_INVALID;
        }
        half[b] = 0.5 * branch_length[b];
    }
    return EPIK_AMD_OK;
}

// the rule's blocked sum: the terms of a block in ascending b, then the blocks in ascending g
struct blocked_sum {
    double acc = 0.0, block = 0.0;
    void add(size_t b, double term)
    {
        block = block + term;
        if ((b + 1) % kDiversityBlock == 0) close();
    }
    void close() { acc = acc + block, block = 0.0; }
    double result(size_t N)
    {
        if (N % kDiversityBlock != 0) close();  // the ragged last block
        return acc;
    }
};

inline double balance(double d)
{
    const double w = std::min(d, 1.0 - d);
    return w > 0.0 ? w : 0.0;
}

}  // namespace

int alpha_indices(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                  const double* branch_length, epik_amd_alpha* alpha, std::string& err)
{
    const size_t S = num_samples, N = num_branches;
    std::vector<double> half;
    if (const int rc = check_tree_lengths(N, first, branch_length, half, err); rc != EPIK_AMD_OK) return rc;
    std::vector<uint64_t> prefix(N + 1);
    for (size_t s = 0; s < S; ++s) {
        const uint64_t* m = mass + s * N;
        prefix[0] = 0;
        for (size_t b = 0; b < N; ++b) prefix[b + 1] = prefix[b] + m[b];
        const uint64_t total = prefix[N];
        if (total == 0) {
            alpha[s] = epik_amd_alpha{-1.0, -1.0, -1.0, -1.0, -1.0};
            continue;
        }
        const double T = (double)total;
        blocked_sum pd, rooted, bw_half, bw_one, quadratic;
        for (size_t b = 0; b < N; ++b) {
            const uint64_t clade = prefix[b + 1] - prefix[first[b]], below = clade - m[b];
            const double C = (double)clade / T, B = (double)below / T, h = half[b];
            const double wb = balance(B), wc = balance(C);
            pd.add(b, h * ((below > 0 && below < total ? 1.0 : 0.0) + (clade > 0 && clade < total ? 1.0 : 0.0)));
            rooted.add(b, h * ((below > 0 ? 1.0 : 0.0) + (clade > 0 ? 1.0 : 0.0)));
            bw_half.add(b, h * (std::sqrt(2.0 * wb) + std::sqrt(2.0 * wc)));
            bw_one.add(b, h * (2.0 * wb + 2.0 * wc));
            quadratic.add(b, h * (B * (1.0 - B) + C * (1.0 - C)));
        }
        alpha[s] = epik_amd_alpha{pd.result(N), rooted.result(N), bw_half.result(N), bw_one.result(N), quadratic.result(N)};
    }
    return EPIK_AMD_OK;
}

int rarefy_depths_valid(uint32_t depth_step, uint32_t num_depths, std::string& err)
{
    if (depth_step < 1 || depth_step > EPIK_AMD_RAREFY_MAX_DEPTH) {
        err = "depth_step = " + std::to_string(depth_step) + " is outside [1, 2^20]";
        return EPIK_AMD_ERR_INVALID;
    }
    if (num_depths < 1 || num_depths > EPIK_AMD_RAREFY_MAX_DEPTHS) {
        err = "num_depths = " + std::to_string(num_depths) + " is outside [1, 256]";
        return EPIK_AMD_ERR_INVALID;
    }
    if ((uint64_t)depth_step * num_depths > EPIK_AMD_RAREFY_MAX_DEPTH) {
        err = "num_depths * depth_step = " + std::to_string((uint64_t)depth_step * num_depths) + " is above 2^20, the deepest depth";
        return EPIK_AMD_ERR_INVALID;
    }
    return EPIK_AMD_OK;
}

int rarefy_curves(const uint64_t* best, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                  const double* branch_length, uint32_t depth_step, uint32_t num_depths, double* curve, std::string& err)
{
    const size_t S = num_samples, N = num_branches, J = num_depths;
    if (const int rc = rarefy_depths_valid(depth_step, num_depths, err); rc != EPIK_AMD_OK) return rc;
    std::vector<double> half;
    if (const int rc = check_tree_lengths(N, first, branch_length, half, err); rc != EPIK_AMD_OK) return rc;
    std::vector<uint64_t> prefix(N + 1), side(4 * N);
    std::vector<double> value(4 * N), factor(4 * N), recip(depth_step);
    std::vector<blocked_sum> sums(2 * J);
    constexpr size_t kTile = 1024;
    for (size_t s = 0; s < S; ++s) {
        const uint64_t* m = best + s * N;
        double* out = curve + s * J * 2;
        std::fill(out, out + 2 * J, -1.0);
        prefix[0] = 0;
        for (size_t b = 0; b < N; ++b) prefix[b + 1] = prefix[b] + m[b];
        const uint64_t n = prefix[N];
        if (n == 0 || n >= (1ull << 53)) continue;  // not rarefiable
        const size_t depths = (size_t)std::min<uint64_t>(J, n / depth_step);  // the j with k_j <= n
        if (depths == 0) continue;
        // the four sides of every branch, side by side: below, all but below, clade, all but clade.  value = Q(side, k) and
        // factor = (double)(n - side - k), kept by subtracting 1.0 (exact below 2^53: the bits of the conversion).  A side
        // with side >= n starts at the factor +0.0, every other side reaches it at k = n - side: the product is a zero from
        // then on, as the rule says, whose sign cannot reach an output; |value| is taken all the same.  The empty side,
        // exactly 1 by the rule, is picked at the output.  One pass over the sides per depth, nothing carried from side to
        // side: the compiler may take several at a time, each operation still rounded on its own.
        for (size_t b = 0; b < N; ++b) {
            const uint64_t cc = prefix[b + 1] - prefix[first[b]], cb = cc - m[b];
            side[b] = cb, side[N + b] = n - cb, side[2 * N + b] = cc, side[3 * N + b] = n - cc;
        }
        for (size_t i = 0; i < 4 * N; ++i) value[i] = 1.0, factor[i] = side[i] < n ? (double)(n - side[i]) : 0.0;
        std::fill(sums.begin(), sums.end(), blocked_sum{});
        const auto chance = [&](size_t i) { return side[i] == 0 ? 1.0 : std::fabs(value[i]); };
        uint64_t k = 0;
        for (size_t j = 0; j < depths; ++j) {
            for (size_t i = 0; i < depth_step; ++i) recip[i] = 1.0 / (double)(n - k - i);  // r_k of the depths up to k_j
            for (size_t tile = 0; tile < 4 * N; tile += kTile) {  // (a tile of sides stays in the first-level cache)
                double *__restrict__ q = value.data() + tile, *__restrict__ f = factor.data() + tile;
                const size_t count = std::min(kTile, 4 * N - tile);
                for (size_t step = 0; step < depth_step; ++step) {
                    const double r = recip[step];
                    for (size_t i = 0; i < count; ++i) q[i] = (q[i] * f[i]) * r, f[i] = f[i] - 1.0;
                }
            }
            k += depth_step;
            for (size_t b = 0; b < N; ++b) {
                const double ru_b = 1.0 - chance(b), ru_c = 1.0 - chance(2 * N + b);
                double uu_b = ru_b - chance(N + b), uu_c = ru_c - chance(3 * N + b);
                if (!(uu_b > 0.0)) uu_b = 0.0;
                if (!(uu_c > 0.0)) uu_c = 0.0;
                sums[2 * j].add(b, half[b] * (uu_b + uu_c));
                sums[2 * j + 1].add(b, half[b] * (ru_b + ru_c));
            }
            out[2 * j] = sums[2 * j].result(N), out[2 * j + 1] = sums[2 * j + 1].result(N);
        }
    }
    return EPIK_AMD_OK;
}

namespace {

inline double na_value()
{
    const uint64_t bits = EPIK_AMD_NA_BITS;
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
}

// the rule's midranks by counting
void midranks(const std::vector<double>& x, std::vector<double>& rank)
{
    const size_t L = x.size();
    rank.resize(L);
    for (size_t j = 0; j < L; ++j) {
        size_t less = 0, equal = 0;
        for (size_t i = 0; i < L; ++i) less += x[i] < x[j], equal += x[i] == x[j];
        rank[j] = (double)less + 0.5 * (double)(equal + 1);
    }
}

// what the rule's Pearson needs of one vector: the mean, the deviations, and their sum of squares (L >= 1)
struct centred {
    double mean = 0.0, ss = 0.0;
    std::vector<double> d;
    void of(const std::vector<double>& x)
    {
        const size_t L = x.size();
        double acc = 0.0;
        for (size_t j = 0; j < L; ++j) acc = acc + x[j];
        mean = acc / (double)L;
        d.resize(L);
        ss = 0.0;
        for (size_t j = 0; j < L; ++j) d[j] = x[j] - mean, ss = ss + d[j] * d[j];
    }
};

double pearson_of(const centred& x, const centred& y)
{
    const size_t L = x.d.size();
    if (L < 3) return na_value();
    double sxy = 0.0;
    for (size_t j = 0; j < L; ++j) sxy = sxy + x.d[j] * y.d[j];
    const double den = std::sqrt(x.ss) * std::sqrt(y.ss);
    if (!(den > 0.0)) return na_value();
    double r = sxy / den;
    if (r < -1.0) r = -1.0;
    if (r > 1.0) r = 1.0;
    return r;
}

// the masses and imbalances of branch b over the samples of `list`
void branch_vectors(const uint64_t* mass, const kr_planes& p, size_t N, size_t b, const std::vector<size_t>& list,
                    std::vector<double>& xm, std::vector<double>& xi)
{
    xm.resize(list.size()), xi.resize(list.size());
    for (size_t j = 0; j < list.size(); ++j) {
        const size_t s = list[j];
        xm[j] = (double)mass[s * N + b] / (double)p.total[s];
        xi[j] = (p.B[s * N + b] + p.C[s * N + b]) - 1.0;
    }
}

}  // namespace

int correlation_columns_valid(const double* meta, uint32_t num_samples, uint32_t num_columns, std::string& err)
{
    if (num_columns < 1 || num_columns > EPIK_AMD_CORRELATION_MAX_COLUMNS) {
        err = "num_columns = " + std::to_string(num_columns) + " is outside [1, 64]";
        return EPIK_AMD_ERR_INVALID;
    }
    for (size_t s = 0; s < num_samples; ++s)
        for (size_t c = 0; c < num_columns; ++c)
            if (std::isinf(meta[s * num_columns + c])) {
                err = "sample " + std::to_string(s) + ", column " + std::to_string(c) + ": the metadata value is infinite";
                return EPIK_AMD_ERR_INVALID;
            }
    return EPIK_AMD_OK;
}

int correlation_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                        const double* meta, uint32_t num_columns, epik_amd_correlation* out, uint32_t* used, std::string& err)
{
    const size_t S = num_samples, N = num_branches, M = num_columns;
    if (const int rc = correlation_columns_valid(meta, num_samples, num_columns, err); rc != EPIK_AMD_OK) return rc;
    kr_planes p;
    if (const int rc = make_planes(mass, S, N, first, nullptr, p, err); rc != EPIK_AMD_OK) return rc;
    const double na = na_value();
    // the columns with the same U_c side by side: mx, dx, sxx and the ranks of x do not depend on y, so they are formed
    // once per set and branch, by the same operations in the same order as for a column on its own
    std::map<std::vector<size_t>, std::vector<size_t>> columns_of;
    for (size_t c = 0; c < M; ++c) {
        std::vector<size_t> list;
        for (size_t s = 0; s < S; ++s)
            if (p.total[s] != 0 && !std::isnan(meta[s * M + c])) list.push_back(s);
        used[c] = (uint32_t)list.size();
        columns_of[std::move(list)].push_back(c);
    }
    std::vector<double> y, ry, xm, xi, rm, ri;
    centred cxm, cxi, crm, cri;
    for (const auto& [list, columns] : columns_of) {
        const size_t L = list.size();
        std::vector<centred> cy(columns.size()), cry(columns.size());
        for (size_t q = 0; q < columns.size() && L >= 3; ++q) {
            y.resize(L);
            for (size_t j = 0; j < L; ++j) y[j] = meta[list[j] * M + columns[q]];
            midranks(y, ry), cy[q].of(y), cry[q].of(ry);
        }
        for (size_t b = 0; b < N; ++b) {
            for (const size_t c : columns) out[c * N + b] = epik_amd_correlation{na, na, na, na};
            if (L < 3) continue;
            const bool inner = first[b] < b;
            branch_vectors(mass, p, N, b, list, xm, xi);
            midranks(xm, rm), cxm.of(xm), crm.of(rm);
            if (inner) midranks(xi, ri), cxi.of(xi), cri.of(ri);
            for (size_t q = 0; q < columns.size(); ++q) {
                epik_amd_correlation& r = out[columns[q] * N + b];
                r.mass_pearson = pearson_of(cxm, cy[q]), r.mass_spearman = pearson_of(crm, cry[q]);
                if (inner) r.imbalance_pearson = pearson_of(cxi, cy[q]), r.imbalance_spearman = pearson_of(cri, cry[q]);
            }
        }
    }
    return EPIK_AMD_OK;
}

int dispersion_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                       epik_amd_dispersion* out, std::string& err)
{
    const size_t S = num_samples, N = num_branches;
    kr_planes p;
    if (const int rc = make_planes(mass, S, N, first, nullptr, p, err); rc != EPIK_AMD_OK) return rc;
    const double na = na_value();
    std::vector<size_t> list;
    for (size_t s = 0; s < S; ++s)
        if (p.total[s] != 0) list.push_back(s);
    const size_t L = list.size();
    std::vector<double> xm, xi;
    centred cm, ci;
    for (size_t b = 0; b < N; ++b) {
        epik_amd_dispersion& r = out[b];
        r = epik_amd_dispersion{na, na, na, na, na, na, na, na};
        if (L == 0) continue;
        branch_vectors(mass, p, N, b, list, xm, xi);
        cm.of(xm);
        r.mass_mean = cm.mean, r.mass_var = cm.ss / (double)L, r.mass_sd = std::sqrt(r.mass_var);
        if (r.mass_mean > 0.0) r.mass_cv = r.mass_sd / r.mass_mean, r.mass_vmr = r.mass_var / r.mass_mean;
        if (!(first[b] < b)) continue;
        ci.of(xi);
        r.imbalance_mean = ci.mean, r.imbalance_var = ci.ss / (double)L, r.imbalance_sd = std::sqrt(r.imbalance_var);
    }
    return EPIK_AMD_OK;
}

namespace {

// [+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?
bool is_number(const std::string& v)
{
    size_t i = 0;
    const auto digits = [&] {
        const size_t from = i;
        while (i < v.size() && v[i] >= '0' && v[i] <= '9') ++i;
        return i - from;
    };
    if (i < v.size() && (v[i] == '+' || v[i] == '-')) ++i;
    const size_t whole = digits();
    size_t fraction = 0;
    if (i < v.size() && v[i] == '.') {
        ++i;
        fraction = digits();
    }
    if (whole + fraction == 0) return false;
    if (i < v.size() && (v[i] == 'e' || v[i] == 'E')) {
        ++i;
        if (i < v.size() && (v[i] == '+' || v[i] == '-')) ++i;
        if (digits() == 0) return false;
    }
    return i == v.size();
}

std::vector<std::string> split_tabs(const std::string& line)
{
    std::vector<std::string> fields;
    size_t from = 0;
    for (;;) {
        const size_t tab = line.find('\t', from);
        fields.push_back(line.substr(from, tab == std::string::npos ? tab : tab - from));
        if (tab == std::string::npos) return fields;
        from = tab + 1;
    }
}

}  // namespace

cohort_metadata read_cohort_metadata(const std::string& file, const std::vector<cohort_sample>& samples)
{
    std::ifstream in(file);
    if (!in) throw std::runtime_error("--cohort-correlation: cannot open the metadata file " + file);
    std::map<std::string, size_t> index;
    for (size_t s = 0; s < samples.size(); ++s) index[samples[s].name] = s;
    cohort_metadata meta;
    std::vector<size_t> seen(samples.size(), 0);  // the line that gave the sample, 0: none yet
    bool have_header = false;
    std::string line;
    for (size_t number = 1; std::getline(in, line); ++number) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::string where = "--cohort-correlation: " + file + " line " + std::to_string(number);
        const auto fields = split_tabs(line);
        if (!have_header) {
            if (fields[0] != "sample") throw std::runtime_error(where + ": the header must begin with 'sample'");
            if (fields.size() < 2 || fields.size() > 1 + EPIK_AMD_CORRELATION_MAX_COLUMNS)
                throw std::runtime_error(where + ": the header names " + std::to_string(fields.size() - 1) +
                                         " columns, not 1 to 64");
            std::set<std::string> names;
            for (size_t c = 1; c < fields.size(); ++c) {
                if (fields[c].empty()) throw std::runtime_error(where + ": column " + std::to_string(c) + " has an empty name");
                if (!names.insert(fields[c]).second)
                    throw std::runtime_error(where + ": the column name '" + fields[c] + "' is given twice");
                meta.columns.push_back(fields[c]);
            }
            meta.values.assign(samples.size() * meta.columns.size(), na_value());
            have_header = true;
            continue;
        }
        const size_t M = meta.columns.size();
        if (fields.size() != M + 1)
            throw std::runtime_error(where + ": " + std::to_string(fields.size()) + " fields, not " + std::to_string(M + 1));
        const auto found = index.find(fields[0]);
        if (found == index.end()) {
            ++meta.skipped;
            continue;
        }
        const size_t s = found->second;
        if (seen[s])
            throw std::runtime_error(where + ": the sample '" + fields[0] + "' is given twice (first on line " +
                                     std::to_string(seen[s]) + ")");
        seen[s] = number;
        for (size_t c = 0; c < M; ++c) {
            const std::string& v = fields[c + 1];
            if (v.empty() || v == "NA") continue;
            const std::string at = where + ", column " + meta.columns[c] + ": ";
            if (!is_number(v)) throw std::runtime_error(at + "'" + v + "' is not a number, empty or NA");
            const double value = std::strtod(v.c_str(), nullptr);
            if (std::isinf(value)) throw std::runtime_error(at + "'" + v + "' overflows a double");
            meta.values[s * M + c] = value;
        }
    }
    if (!have_header) throw std::runtime_error("--cohort-correlation: " + file + " has no header line");
    for (size_t s = 0; s < samples.size(); ++s)
        if (!seen[s]) throw std::runtime_error("--cohort-correlation: " + file + " has no line for the sample '" + samples[s].name + "'");
    return meta;
}

namespace {

// the rule's key of position i in permutation p: the splitmix64 finaliser of a counter
inline uint64_t permanova_key(uint64_t seed, uint32_t p, uint32_t i)
{
    uint64_t z = seed + (((uint64_t)p << 32) | i) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The arrangements sigma_p of the strata rule (include/epik_amd.h) over n positions: what the four permutation tests share.
// `strata` is by sample, or null for one stratum, and sample[i] the sample of position i.  home[] lists the positions by
// (stratum, position); the positions sorted by (stratum, key, position) take its entries slot by slot, so a position gets
// the w-th member of its own stratum.  With one stratum sigma_p(i) = rank_p(i).
struct arrangements {
    std::vector<uint32_t> h, home, sigma;
    std::vector<std::tuple<uint32_t, uint64_t, uint32_t>> keys;
    template <class Sample>
    arrangements(const uint32_t* strata, size_t n, Sample sample) : h(n, 0), home(n), sigma(n), keys(n)
    {
        for (size_t i = 0; i < n; ++i) home[i] = (uint32_t)i, h[i] = strata ? strata[sample(i)] : 0;
        std::stable_sort(home.begin(), home.end(), [&](uint32_t a, uint32_t b) { return h[a] < h[b]; });
    }
    const std::vector<uint32_t>& of(uint64_t seed, uint32_t p)
    {
        const size_t n = h.size();
        for (uint32_t i = 0; i < n; ++i) keys[i] = {h[i], permanova_key(seed, p, i), i};
        std::sort(keys.begin(), keys.end());
        for (size_t r = 0; r < n; ++r) sigma[std::get<2>(keys[r])] = home[r];
        return sigma;
    }
};

// SSW(mu) over the compact block A[n][n]: the rule's three chains; W_g / n_g into `terms` where asked for
double permanova_ssw(const std::vector<double>& A, size_t n, const std::vector<uint32_t>& mu, const std::vector<uint32_t>& size,
                     std::vector<double>& t, double* terms)
{
    for (size_t i = 0; i < n; ++i) {
        double acc = 0.0;
        for (size_t j = i + 1; j < n; ++j)
            if (mu[j] == mu[i]) acc = acc + A[i * n + j];
        t[i] = acc;
    }
    double ssw = 0.0;
    for (size_t g = 0; g < size.size(); ++g) {
        double w = 0.0;
        for (size_t i = 0; i < n; ++i)
            if (mu[i] == g) w = w + t[i];
        const double term = w / (double)size[g];
        if (terms) terms[g] = term;
        ssw = ssw + term;
    }
    return ssw;
}

// one test of the rule: the samples idx[n] with the groups lam[n] of sizes size[G]
void permanova_test(const double* kr, size_t S, const std::vector<uint32_t>& idx, const std::vector<uint32_t>& lam,
                    const std::vector<uint32_t>& size, uint32_t P, uint64_t seed, epik_amd_permanova& rec, double* ssw, double* terms,
                    const uint32_t* strata)
{
    const size_t n = idx.size(), G = size.size();
    rec.used = (uint32_t)n, rec.groups = (uint32_t)G;
    if (G < 2 || n < G + 1) return;
    std::vector<double> A(n * n), t(n);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) {
            const double d = kr[(size_t)idx[i] * S + idx[j]];
            A[i * n + j] = d * d;
        }
    const double T = permanova_ssw(A, n, std::vector<uint32_t>(n, 0), std::vector<uint32_t>(1, 1), t, nullptr);  // (W_0 / 1.0)
    const double ssw0 = permanova_ssw(A, n, lam, size, t, terms);
    if (ssw) ssw[0] = ssw0;
    rec.ss_total = T / (double)n, rec.ss_within = ssw0;
    const double among = rec.ss_total - ssw0;
    if (rec.ss_total != 0.0) {
        rec.r2 = among / rec.ss_total;
        if (ssw0 != 0.0) rec.f = (among / (double)(G - 1)) / (ssw0 / (double)(n - G));
    }
    arrangements arrange(strata, n, [&](size_t i) { return idx[i]; });
    std::vector<uint32_t> mu(n);
    uint64_t at_most = 0;
    for (uint32_t p = 1; p <= P; ++p) {
        const std::vector<uint32_t>& sigma = arrange.of(seed, p);
        for (size_t i = 0; i < n; ++i) mu[i] = lam[sigma[i]];
        const double v = permanova_ssw(A, n, mu, size, t, nullptr);
        if (ssw) ssw[p] = v;
        at_most += v <= ssw0;
    }
    rec.at_most = at_most;
    rec.p = (double)(1 + at_most) / (double)(P + 1);
}

}  // namespace

int permanova_arguments_valid(const uint32_t* labels, uint32_t num_samples, uint32_t num_columns, uint32_t num_permutations,
                              bool pairwise, std::string& err)
{
    if (num_columns < 1 || num_columns > EPIK_AMD_PERMANOVA_MAX_COLUMNS) {
        err = "num_columns = " + std::to_string(num_columns) + " is outside [1, 64]";
        return EPIK_AMD_ERR_INVALID;
    }
    if (num_permutations < 1 || num_permutations > EPIK_AMD_PERMANOVA_MAX_PERMUTATIONS) {
        err = "num_permutations = " + std::to_string(num_permutations) + " is outside [1, 999999]";
        return EPIK_AMD_ERR_INVALID;
    }
    for (size_t c = 0; c < num_columns; ++c) {
        std::set<uint32_t> distinct;
        for (size_t s = 0; s < num_samples; ++s) {
            const uint32_t v = labels[s * num_columns + c];
            if (v == EPIK_AMD_PERMANOVA_MISSING) continue;
            if (v >= EPIK_AMD_PERMANOVA_MAX_GROUPS) {
                err = "sample " + std::to_string(s) + ", column " + std::to_string(c) + ": the label " + std::to_string(v) +
                      " is not below 256";
                return EPIK_AMD_ERR_INVALID;
            }
            distinct.insert(v);
        }
        if (pairwise && distinct.size() > EPIK_AMD_PERMANOVA_MAX_PAIR_GROUPS) {
            err = "column " + std::to_string(c) + ": " + std::to_string(distinct.size()) + " distinct labels, pairwise takes 32 at the most";
            return EPIK_AMD_ERR_INVALID;
        }
    }
    return EPIK_AMD_OK;
}

int permanova_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const uint32_t* labels,
                            uint32_t num_columns, uint32_t num_permutations, uint64_t seed, bool pairwise, epik_amd_permanova* out,
                            double* ssw, double* group_ss, std::string& err, const uint32_t* strata)
{
    const size_t S = num_samples, M = num_columns, P = num_permutations;
    if (const int rc = permanova_arguments_valid(labels, num_samples, num_columns, num_permutations, pairwise, err); rc != EPIK_AMD_OK)
        return rc;
    const size_t slots = 1 + (pairwise ? EPIK_AMD_PERMANOVA_PAIR_SLOTS : 0);
    const double na = na_value();
    for (size_t e = 0; e < M * slots; ++e) out[e] = epik_amd_permanova{0, 0, 0, na, na, na, na, na};
    if (ssw) std::fill(ssw, ssw + M * slots * (P + 1), na);
    if (group_ss) std::fill(group_ss, group_ss + M * EPIK_AMD_PERMANOVA_MAX_GROUPS, na);
    for (size_t c = 0; c < M; ++c) {
        std::vector<uint32_t> idx, lam, size, group_of(EPIK_AMD_PERMANOVA_MAX_GROUPS, EPIK_AMD_PERMANOVA_MISSING);
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (totals[s] == 0 || v == EPIK_AMD_PERMANOVA_MISSING) continue;
            if (group_of[v] == EPIK_AMD_PERMANOVA_MISSING) group_of[v] = (uint32_t)size.size(), size.push_back(0);
            idx.push_back((uint32_t)s), lam.push_back(group_of[v]), ++size[group_of[v]];
        }
        permanova_test(kr, S, idx, lam, size, num_permutations, seed, out[c * slots], ssw ? ssw + c * slots * (P + 1) : nullptr,
                       group_ss ? group_ss + c * EPIK_AMD_PERMANOVA_MAX_GROUPS : nullptr, strata);
        if (!pairwise) continue;
        for (size_t h = 1; h < size.size(); ++h)
            for (size_t g = 0; g < h; ++g) {
                std::vector<uint32_t> sub, two;
                for (size_t i = 0; i < idx.size(); ++i)
                    if (lam[i] == g || lam[i] == h) sub.push_back(idx[i]), two.push_back(lam[i] == h);
                const size_t slot = c * slots + 1 + h * (h - 1) / 2 + g;
                permanova_test(kr, S, sub, two, {size[g], size[h]}, num_permutations, seed, out[slot],
                               ssw ? ssw + slot * (P + 1) : nullptr, nullptr, strata);
            }
    }
    return EPIK_AMD_OK;
}

int permanova_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                      const double* branch_length, const uint32_t* labels, uint32_t num_columns, uint32_t num_permutations,
                      uint64_t seed, bool pairwise, epik_amd_permanova* out, double* ssw, double* group_ss, std::string& err,
                      uint32_t metric, const uint32_t* strata)
{
    const size_t S = num_samples, N = num_branches;
    if (const int rc = permanova_arguments_valid(labels, num_samples, num_columns, num_permutations, pairwise, err); rc != EPIK_AMD_OK)
        return rc;
    std::vector<double> kr(S * S);
    if (const int rc = distance_matrix(mass, num_samples, num_branches, first, branch_length, metric, kr.data(), err); rc != EPIK_AMD_OK)
        return rc;
    std::vector<uint64_t> totals(S, 0);
    for (size_t s = 0; s < S; ++s)
        for (size_t b = 0; b < N; ++b) totals[s] += mass[s * N + b];
    return permanova_records_of_kr(kr.data(), totals.data(), num_samples, labels, num_columns, num_permutations, seed, pairwise, out,
                                   ssw, group_ss, err, strata);
}

int pcoa_components_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, uint32_t num_components, double* mu,
                          double* coord, epik_amd_pcoa_info* info, std::string& err)
{
    const size_t S = num_samples, K = num_components;
    if (K < 1 || K > EPIK_AMD_PCOA_MAX_COMPONENTS) {
        err = "num_components = " + std::to_string(K) + " is outside [1, 64]";
        return EPIK_AMD_ERR_INVALID;
    }
    std::vector<size_t> used;
    for (size_t s = 0; s < S; ++s)
        if (totals[s] != 0) used.push_back(s);
    const size_t L = used.size(), Kc = std::min(K, L);
    // the squared distances, Gower's centring, the scale and the trace
    std::vector<double> A(L * L, 0.0), V(L * L, 0.0), r(L);
    for (size_t i = 0; i < L; ++i)
        for (size_t j = 0; j < L; ++j) {
            const double d = kr[used[i] * S + used[j]];
            A[i * L + j] = d * d;
        }
    double g = 0.0;
    for (size_t i = 0; i < L; ++i) {
        double acc = 0.0;
        for (size_t j = 0; j < L; ++j) acc = acc + A[j * L + i];  // (KR[u_j][u_i], the element the device's lanes read)
        r[i] = acc / (double)L;
        g = g + r[i];
    }
    if (L) g = g / (double)L;
    for (size_t i = 0; i < L; ++i)
        for (size_t j = i; j < L; ++j) A[i * L + j] = A[j * L + i] = -0.5 * (((A[i * L + j] - r[i]) - r[j]) + g);
    double scale = 0.0, trace = 0.0;
    for (size_t j = 0; j < L; ++j) {
        if (std::fabs(A[j * L + j]) > scale) scale = std::fabs(A[j * L + j]);
        trace = trace + A[j * L + j];
        V[j * L + j] = 1.0;
    }
    uint32_t sweeps = 0, converged = 0;
    jacobi_sweeps(A, V, L, std::ldexp(1.0, -52) * scale, sweeps, converged);
    // the axes: by (mu descending, j ascending), all L of them
    std::vector<size_t> column(L);
    for (size_t j = 0; j < L; ++j) {
        size_t rank = 0;
        for (size_t i = 0; i < L; ++i)
            rank += A[i * L + i] > A[j * L + j] || (A[i * L + i] == A[j * L + j] && i < j) ? 1 : 0;
        column[rank] = j;
    }
    std::fill(mu, mu + S, 0.0), std::fill(coord, coord + S * K, 0.0);
    const double floor_mu = std::ldexp(1.0, -40) * scale;
    double pos = 0.0, neg = 0.0;
    for (size_t k = 0; k < L; ++k) {
        const size_t jk = column[k];
        mu[k] = A[jk * L + jk];
        if (mu[k] > floor_mu) pos = pos + mu[k];
        if (mu[k] < -floor_mu) neg = neg + mu[k];
        if (k >= Kc || !(mu[k] > floor_mu)) continue;
        const double root = std::sqrt(mu[k]);
        size_t at = 0;
        for (size_t j = 0; j < L; ++j)
            if (std::fabs(V[j * L + jk]) > std::fabs(V[at * L + jk])) at = j;
        const double sign = V[at * L + jk] < 0.0 ? -1.0 : 1.0;
        for (size_t j = 0; j < L; ++j) coord[used[j] * K + k] = sign * (V[j * L + jk] * root);
    }
    *info = epik_amd_pcoa_info{(uint32_t)L, (uint32_t)Kc, sweeps, converged, trace, scale, pos, neg};
    return EPIK_AMD_OK;
}

int pcoa_components(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                    const double* branch_length, uint32_t num_components, double* mu, double* coord, epik_amd_pcoa_info* info,
                    std::string& err, uint32_t metric)
{
    const size_t S = num_samples, N = num_branches;
    if (num_components < 1 || num_components > EPIK_AMD_PCOA_MAX_COMPONENTS) {
        err = "num_components = " + std::to_string(num_components) + " is outside [1, 64]";
        return EPIK_AMD_ERR_INVALID;
    }
    std::vector<double> kr(S * S);
    if (const int rc = distance_matrix(mass, num_samples, num_branches, first, branch_length, metric, kr.data(), err); rc != EPIK_AMD_OK)
        return rc;
    std::vector<uint64_t> totals(S, 0);
    for (size_t s = 0; s < S; ++s)
        for (size_t b = 0; b < N; ++b) totals[s] += mass[s * N + b];
    return pcoa_components_of_kr(kr.data(), totals.data(), num_samples, num_components, mu, coord, info, err);
}

namespace {

// the rule's midranks by sorting: the same two counts as midranks(), found in another way (exact half-integers)
void midranks_sorted(const std::vector<double>& x, std::vector<uint32_t>& order, std::vector<double>& rank)
{
    const size_t L = x.size();
    order.resize(L), rank.resize(L);
    for (size_t j = 0; j < L; ++j) order[j] = (uint32_t)j;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return x[a] < x[b]; });
    for (size_t from = 0; from < L;) {
        size_t to = from + 1;
        while (to < L && x[order[to]] == x[order[from]]) ++to;
        const double r = (double)from + 0.5 * (double)(to - from + 1);
        for (size_t k = from; k < to; ++k) rank[order[k]] = r;
        from = to;
    }
}

// A(mu) of the rule for the deviations d: the chains S_g in `sums`, then the chain over g
inline double edgetest_among(const double* d, const uint8_t* mu, size_t L, const std::vector<uint32_t>& size, double* sums)
{
    const size_t G = size.size();
    for (size_t g = 0; g < G; ++g) sums[g] = 0.0;
    for (size_t i = 0; i < L; ++i) sums[mu[i]] = sums[mu[i]] + d[i];
    double among = 0.0;
    for (size_t g = 0; g < G; ++g) among = among + (sums[g] * sums[g]) / (double)size[g];
    return among;
}

}  // namespace

int edgetest_arguments_valid(const uint32_t* labels, uint32_t num_samples, uint32_t num_columns, uint32_t num_permutations,
                             std::string& err)
{
    if (num_columns < 1 || num_columns > EPIK_AMD_EDGETEST_MAX_COLUMNS) {
        err = "num_columns = " + std::to_string(num_columns) + " is outside [1, 64]";
        return EPIK_AMD_ERR_INVALID;
    }
    if (num_permutations < 1 || num_permutations > EPIK_AMD_EDGETEST_MAX_PERMUTATIONS) {
        err = "num_permutations = " + std::to_string(num_permutations) + " is outside [1, 999999]";
        return EPIK_AMD_ERR_INVALID;
    }
    for (size_t s = 0; s < num_samples; ++s)
        for (size_t c = 0; c < num_columns; ++c) {
            const uint32_t v = labels[s * num_columns + c];
            if (v != EPIK_AMD_EDGETEST_MISSING && v >= EPIK_AMD_EDGETEST_MAX_GROUPS) {
                err = "sample " + std::to_string(s) + ", column " + std::to_string(c) + ": the label " + std::to_string(v) +
                      " is not below 32";
                return EPIK_AMD_ERR_INVALID;
            }
        }
    return EPIK_AMD_OK;
}

int edgetest_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                     const uint32_t* labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed, epik_amd_edgetest* out,
                     double* stat, double* max, std::string& err, const uint32_t* strata)
{
    constexpr size_t F = EPIK_AMD_EDGETEST_FAMILIES;
    const size_t S = num_samples, N = num_branches, M = num_columns, P = num_permutations, row = P + 1;
    if (const int rc = edgetest_arguments_valid(labels, num_samples, num_columns, num_permutations, err); rc != EPIK_AMD_OK) return rc;
    kr_planes planes;
    if (const int rc = make_planes(mass, S, N, first, nullptr, planes, err); rc != EPIK_AMD_OK) return rc;
    const double na = na_value();
    const epik_amd_edgetest_family none{na, na, na, na, 0, 0};
    if (stat) std::fill(stat, stat + M * F * N * row, na);
    if (max) std::fill(max, max + M * F * row, na);
    for (size_t c = 0; c < M; ++c) {
        std::vector<size_t> list;
        std::vector<uint32_t> lam, size, group_of(EPIK_AMD_EDGETEST_MAX_GROUPS, EPIK_AMD_EDGETEST_MISSING);
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (planes.total[s] == 0 || v == EPIK_AMD_EDGETEST_MISSING) continue;
            if (group_of[v] == EPIK_AMD_EDGETEST_MISSING) group_of[v] = (uint32_t)size.size(), size.push_back(0);
            list.push_back(s), lam.push_back(group_of[v]), ++size[group_of[v]];
        }
        const size_t L = list.size(), G = size.size();
        for (size_t b = 0; b < N; ++b) {
            epik_amd_edgetest& r = out[c * N + b];
            r.used = (uint32_t)L, r.groups = (uint32_t)G, r.top_mass = r.top_imbalance = EPIK_AMD_EDGETEST_MISSING;
            for (size_t f = 0; f < F; ++f) r.family[f] = none;
        }
        if (G < 2 || L < G + 1) continue;
        // the labellings in chunks of permutations, a byte a position: the vectors of a branch are formed once a chunk
        const size_t chunk = std::max<size_t>(1, ((size_t)64 << 20) / L);
        std::vector<uint8_t> mu(std::min(chunk, row) * L);
        arrangements arrange(strata, L, [&](size_t i) { return list[i]; });
        std::vector<double> mmax(F * row, 0.0), sums(G), rank;
        std::vector<char> any(F, 0);
        std::vector<double> x[F];
        std::vector<uint32_t> order;
        centred dev[F];
        for (size_t p0 = 0; p0 < row; p0 += chunk) {
            const size_t np = std::min(chunk, row - p0);
            for (size_t k = 0; k < np; ++k) {
                uint8_t* m = mu.data() + k * L;
                const uint32_t p = (uint32_t)(p0 + k);
                if (p == 0) {
                    for (size_t i = 0; i < L; ++i) m[i] = (uint8_t)lam[i];
                    continue;
                }
                const std::vector<uint32_t>& sigma = arrange.of(seed, p);
                for (size_t i = 0; i < L; ++i) m[i] = (uint8_t)lam[sigma[i]];
            }
            for (size_t b = 0; b < N; ++b) {
                epik_amd_edgetest& r = out[c * N + b];
                const bool inner = first[b] < b;
                branch_vectors(mass, planes, N, b, list, x[0], x[2]);
                midranks_sorted(x[0], order, x[1]);
                if (inner) midranks_sorted(x[2], order, x[3]);
                for (size_t f = 0; f < (inner ? F : 2); ++f) {
                    dev[f].of(x[f]);
                    const double sxx = dev[f].ss;
                    if (!(sxx > 0.0)) continue;
                    const double* d = dev[f].d.data();
                    epik_amd_edgetest_family& fam = r.family[f];
                    if (p0 == 0) {
                        const double among = edgetest_among(d, mu.data(), L, size, sums.data());
                        fam.eta2 = among / sxx, fam.at_least = 0, fam.max_at_least = 0;
                        if (f % 2 == 0) {
                            const double ssw = sxx - among;
                            if (ssw > 0.0) fam.stat = (among / (double)(G - 1)) / (ssw / (double)(L - G));
                            uint32_t top = 0;
                            double best = sums[0] / (double)size[0];
                            for (size_t g = 1; g < G; ++g)
                                if (const double mean = sums[g] / (double)size[g]; mean > best) best = mean, top = (uint32_t)g;
                            (f == 0 ? r.top_mass : r.top_imbalance) = top;
                        } else {
                            fam.stat = (double)(L - 1) * fam.eta2;
                        }
                        any[f] = 1;
                    }
                    uint64_t at_least = 0;
                    for (size_t k = 0; k < np; ++k) {
                        const double eta = edgetest_among(d, mu.data() + k * L, L, size, sums.data()) / sxx;
                        if (stat) stat[((c * F + f) * N + b) * row + p0 + k] = eta;
                        if (eta > mmax[f * row + p0 + k]) mmax[f * row + p0 + k] = eta;
                        at_least += p0 + k >= 1 && eta >= fam.eta2;
                    }
                    fam.at_least += at_least;
                }
            }
        }
        // max_at_least by a search in the sorted maxima: a count, exact however it is found
        for (size_t f = 0; f < F; ++f) {
            if (!any[f]) continue;
            if (max) std::copy(mmax.begin() + f * row, mmax.begin() + (f + 1) * row, max + (c * F + f) * row);
            std::vector<double> sorted(mmax.begin() + f * row + 1, mmax.begin() + (f + 1) * row);
            std::sort(sorted.begin(), sorted.end());
            for (size_t b = 0; b < N; ++b) {
                epik_amd_edgetest_family& fam = out[c * N + b].family[f];
                if (std::isnan(fam.eta2)) continue;
                fam.max_at_least = (uint64_t)(sorted.end() - std::lower_bound(sorted.begin(), sorted.end(), fam.eta2));
                fam.p = (double)(1 + fam.at_least) / (double)(P + 1);
                fam.p_adj = (double)(1 + fam.max_at_least) / (double)(P + 1);
            }
        }
    }
    return EPIK_AMD_OK;
}

namespace {

// what the tests of a column share under the PERMDISP rule: z, r and the clipped flags by position
struct permdisp_column {
    std::vector<double> z, r;
    std::vector<char> clip;
    std::vector<uint32_t> strata;  // by position, or empty: one stratum
};

// one test of the PERMDISP rule: the column's positions pos[n] with the groups lam[n] of sizes size[G]
void permdisp_test(const permdisp_column& col, const std::vector<uint32_t>& pos, const std::vector<uint8_t>& lam,
                   const std::vector<uint32_t>& size, uint32_t P, uint64_t seed, epik_amd_permdisp& rec, double* stat)
{
    const size_t n = pos.size(), G = size.size();
    rec.used = (uint32_t)n, rec.groups = (uint32_t)G;
    for (size_t i = 0; i < n; ++i) rec.clipped += col.clip[pos[i]] != 0;
    if (G < 2 || n < G + 1) return;
    std::vector<double> x(n), sums(G);
    for (size_t i = 0; i < n; ++i) x[i] = col.z[pos[i]];
    centred dz, dr;
    dz.of(x);
    if (!(dz.ss > 0.0)) return;
    const double among = edgetest_among(dz.d.data(), lam.data(), n, size, sums.data());
    rec.eta2 = among / dz.ss;
    const double ssw = dz.ss - among;
    if (ssw > 0.0) rec.f = (among / (double)(G - 1)) / (ssw / (double)(n - G));
    if (stat) stat[0] = rec.eta2;
    for (size_t i = 0; i < n; ++i) x[i] = col.r[pos[i]];
    dr.of(x);
    if (!(dr.ss > 0.0)) {  // nothing to permute: every permuted statistic is a tie
        rec.at_least = P;
        if (stat) std::fill(stat + 1, stat + 1 + P, rec.eta2);
    } else {
        arrangements arrange(col.strata.empty() ? nullptr : col.strata.data(), n, [&](size_t i) { return pos[i]; });
        std::vector<uint8_t> mu(n);
        for (uint32_t p = 1; p <= P; ++p) {
            const std::vector<uint32_t>& sigma = arrange.of(seed, p);
            for (size_t i = 0; i < n; ++i) mu[i] = lam[sigma[i]];
            const double eta = edgetest_among(dr.d.data(), mu.data(), n, size, sums.data()) / dr.ss;
            if (stat) stat[p] = eta;
            rec.at_least += eta >= rec.eta2;
        }
    }
    rec.p = (double)(1 + rec.at_least) / (double)(P + 1);
}

}  // namespace

int permdisp_arguments_valid(const uint32_t* labels, uint32_t num_samples, uint32_t num_columns, uint32_t num_permutations,
                             std::string& err)
{
    return edgetest_arguments_valid(labels, num_samples, num_columns, num_permutations, err);  // (the same caps)
}

int permdisp_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const uint32_t* labels,
                           uint32_t num_columns, uint32_t num_permutations, uint64_t seed, bool pairwise, epik_amd_permdisp* out,
                           double* stat, double* group_mean, double* z, std::string& err, const uint32_t* strata)
{
    const size_t S = num_samples, M = num_columns, P = num_permutations;
    if (const int rc = permdisp_arguments_valid(labels, num_samples, num_columns, num_permutations, err); rc != EPIK_AMD_OK) return rc;
    const size_t slots = 1 + (pairwise ? EPIK_AMD_PERMDISP_PAIR_SLOTS : 0);
    const double na = na_value();
    for (size_t e = 0; e < M * slots; ++e) out[e] = epik_amd_permdisp{0, 0, 0, 0, 0, na, na, na};
    if (stat) std::fill(stat, stat + M * slots * (P + 1), na);
    std::fill(group_mean, group_mean + M * EPIK_AMD_PERMDISP_MAX_GROUPS, na);
    std::fill(z, z + M * S, na);
    for (size_t c = 0; c < M; ++c) {
        std::vector<uint32_t> idx, size, group_of(EPIK_AMD_PERMDISP_MAX_GROUPS, EPIK_AMD_PERMDISP_MISSING);
        std::vector<uint8_t> lam;
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (totals[s] == 0 || v == EPIK_AMD_PERMDISP_MISSING) continue;
            if (group_of[v] == EPIK_AMD_PERMDISP_MISSING) group_of[v] = (uint32_t)size.size(), size.push_back(0);
            idx.push_back((uint32_t)s), lam.push_back((uint8_t)group_of[v]), ++size[group_of[v]];
        }
        const size_t L = idx.size(), G = size.size();
        // the distances to the centroids: t_i and W_g are PERMANOVA's chains under lambda; A2[i][j] is the square of KR[u_j][u_i]
        const auto a2 = [&](size_t i, size_t j) {
            const double d = kr[(size_t)idx[j] * S + idx[i]];
            return d * d;
        };
        std::vector<double> w(G, 0.0), mean(G, 0.0), m(L);
        for (size_t i = 0; i < L; ++i) {
            double t = 0.0, all = 0.0;
            for (size_t j = 0; j < L; ++j) {
                if (lam[j] != lam[i]) continue;
                const double a = a2(i, j);
                all = all + a;
                if (j > i) t = t + a;
            }
            w[lam[i]] = w[lam[i]] + t;
            m[i] = all / (double)size[lam[i]];
        }
        permdisp_column col;
        col.z.resize(L), col.r.resize(L), col.clip.resize(L);
        if (strata)
            for (size_t i = 0; i < L; ++i) col.strata.push_back(strata[idx[i]]);
        for (size_t i = 0; i < L; ++i) {
            const uint32_t g = lam[i];
            const double z2 = m[i] - (w[g] / (double)size[g]) / (double)size[g];
            col.clip[i] = z2 < 0.0;
            col.z[i] = z2 > 0.0 ? std::sqrt(z2) : 0.0;
            mean[g] = mean[g] + col.z[i];
            z[c * S + idx[i]] = col.z[i];
        }
        for (size_t g = 0; g < G; ++g) group_mean[c * EPIK_AMD_PERMDISP_MAX_GROUPS + g] = mean[g] = mean[g] / (double)size[g];
        for (size_t i = 0; i < L; ++i) col.r[i] = col.z[i] - mean[lam[i]];
        std::vector<uint32_t> pos(L);
        for (size_t i = 0; i < L; ++i) pos[i] = (uint32_t)i;
        permdisp_test(col, pos, lam, size, num_permutations, seed, out[c * slots], stat ? stat + c * slots * (P + 1) : nullptr);
        if (!pairwise) continue;
        for (size_t h = 1; h < G; ++h)
            for (size_t g = 0; g < h; ++g) {
                std::vector<uint32_t> sub;
                std::vector<uint8_t> two;
                for (size_t i = 0; i < L; ++i)
                    if (lam[i] == g || lam[i] == h) sub.push_back((uint32_t)i), two.push_back(lam[i] == h);
                const size_t slot = c * slots + 1 + h * (h - 1) / 2 + g;
                permdisp_test(col, sub, two, {size[g], size[h]}, num_permutations, seed, out[slot],
                              stat ? stat + slot * (P + 1) : nullptr);
            }
    }
    return EPIK_AMD_OK;
}

int permdisp_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                     const double* branch_length, const uint32_t* labels, uint32_t num_columns, uint32_t num_permutations,
                     uint64_t seed, bool pairwise, epik_amd_permdisp* out, double* stat, double* group_mean, double* z, std::string& err,
                     uint32_t metric, const uint32_t* strata)
{
    const size_t S = num_samples, N = num_branches;
    if (const int rc = permdisp_arguments_valid(labels, num_samples, num_columns, num_permutations, err); rc != EPIK_AMD_OK) return rc;
    std::vector<double> kr(S * S);
    if (const int rc = distance_matrix(mass, num_samples, num_branches, first, branch_length, metric, kr.data(), err); rc != EPIK_AMD_OK)
        return rc;
    std::vector<uint64_t> totals(S, 0);
    for (size_t s = 0; s < S; ++s)
        for (size_t b = 0; b < N; ++b) totals[s] += mass[s * N + b];
    return permdisp_records_of_kr(kr.data(), totals.data(), num_samples, labels, num_columns, num_permutations, seed, pairwise, out,
                                  stat, group_mean, z, err, strata);
}

int model_arguments_valid(const uint32_t* kind, const uint32_t* labels, const double* values, uint32_t num_samples,
                          uint32_t num_terms, uint32_t num_permutations, std::string& err)
{
    const size_t S = num_samples, T = num_terms;
    if (num_terms < 1 || num_terms > EPIK_AMD_MODEL_MAX_TERMS) {
        err = "num_terms = " + std::to_string(num_terms) + " is outside [1, 16]";
        return EPIK_AMD_ERR_INVALID;
    }
    if (num_permutations < 1 || num_permutations > EPIK_AMD_MODEL_MAX_PERMUTATIONS) {
        err = "num_permutations = " + std::to_string(num_permutations) + " is outside [1, 999999]";
        return EPIK_AMD_ERR_INVALID;
    }
    size_t columns = 0;
    for (size_t t = 0; t < T; ++t) {
        if (kind[t] > 1) {
            err = "term " + std::to_string(t) + ": the kind " + std::to_string(kind[t]) + " is neither 0 (a factor) nor 1 (numeric)";
            return EPIK_AMD_ERR_INVALID;
        }
        std::set<uint32_t> distinct;
        for (size_t s = 0; s < S; ++s) {
            if (kind[t]) {
                if (std::isinf(values[s * T + t])) {
                    err = "sample " + std::to_string(s) + ", term " + std::to_string(t) + ": the value is infinite";
                    return EPIK_AMD_ERR_INVALID;
                }
                continue;
            }
            const uint32_t v = labels[s * T + t];
            if (v == EPIK_AMD_MODEL_MISSING) continue;
            if (v >= EPIK_AMD_MODEL_MAX_GROUPS) {
                err = "sample " + std::to_string(s) + ", term " + std::to_string(t) + ": the label " + std::to_string(v) +
                      " is not below 32";
                return EPIK_AMD_ERR_INVALID;
            }
            distinct.insert(v);
        }
        columns += kind[t] ? 1 : distinct.empty() ? 0 : distinct.size() - 1;
    }
    if (columns > EPIK_AMD_MODEL_MAX_COLUMNS) {
        err = "the design has " + std::to_string(columns) + " columns, a model takes 64 at the most";
        return EPIK_AMD_ERR_INVALID;
    }
    return EPIK_AMD_OK;
}

namespace {

// Steps 1, 3 and 4 of the sequential model's rule, which the edge model shares word for word: the complete cases with mass, the
// centred columns in term order and the basis by classical Gram-Schmidt twice.  Nothing here depends on the response.
struct design_basis {
    std::vector<size_t> used;            // U, in list order
    std::vector<std::vector<double>> Q;  // the accepted columns, in order
    std::vector<uint32_t> df, columns;   // [T + 1]: of a term, and of the whole model
    size_t C = 0;
    int64_t df_res = 0;
    design_basis(const uint64_t* totals, size_t S, const uint32_t* kind, const uint32_t* labels, const double* values, size_t T,
                 uint8_t* aliased)
        : df(T + 1, 0), columns(T + 1, 0)
    {
        // 1: the complete cases with mass
        for (size_t s = 0; s < S; ++s) {
            bool complete = totals[s] != 0;
            for (size_t t = 0; t < T && complete; ++t)
                complete = kind[t] ? !std::isnan(values[s * T + t]) : labels[s * T + t] != EPIK_AMD_MODEL_MISSING;
            if (complete) used.push_back(s);
        }
        const size_t L = used.size();
        // 3 and 4: the columns in term order, centred, and the basis by classical Gram-Schmidt twice
        std::fill(aliased, aliased + EPIK_AMD_MODEL_MAX_COLUMNS, (uint8_t)0);
        std::vector<double> v(L), h;
        for (size_t t = 0; t < T; ++t) {
            std::vector<uint32_t> lam(L, 0), group_of(EPIK_AMD_MODEL_MAX_GROUPS, EPIK_AMD_MODEL_MISSING);
            uint32_t G = 0;
            if (!kind[t])
                for (size_t i = 0; i < L; ++i) {
                    const uint32_t label = labels[used[i] * T + t];
                    if (group_of[label] == EPIK_AMD_MODEL_MISSING) group_of[label] = G++;
                    lam[i] = group_of[label];
                }
            const uint32_t width = kind[t] ? 1 : G ? G - 1 : 0;
            for (uint32_t w = 0; w < width; ++w, ++C) {
                ++columns[t];
                for (size_t i = 0; i < L; ++i) v[i] = kind[t] ? values[used[i] * T + t] : lam[i] == w + 1 ? 1.0 : 0.0;
                double n0 = 0.0;
                if (L) {
                    double acc = 0.0;
                    for (size_t i = 0; i < L; ++i) acc = acc + v[i];
                    const double mean = acc / (double)L;
                    for (size_t i = 0; i < L; ++i) v[i] = v[i] - mean, n0 = n0 + v[i] * v[i];
                }
                for (int pass = 0; pass < 2; ++pass) {
                    h.assign(Q.size(), 0.0);
                    for (size_t k = 0; k < Q.size(); ++k)
                        for (size_t i = 0; i < L; ++i) h[k] = h[k] + Q[k][i] * v[i];
                    for (size_t i = 0; i < L; ++i)
                        for (size_t k = 0; k < Q.size(); ++k) v[i] = v[i] - h[k] * Q[k][i];
                }
                double n1 = 0.0;
                for (size_t i = 0; i < L; ++i) n1 = n1 + v[i] * v[i];
                if (n0 > 0.0 && n1 > std::ldexp(1.0, -40) * n0) {
                    const double root = std::sqrt(n1);
                    Q.emplace_back(L);
                    for (size_t i = 0; i < L; ++i) Q.back()[i] = v[i] / root;
                    ++df[t];
                } else {
                    aliased[C] = 1;
                }
            }
        }
        const size_t R = Q.size();
        df[T] = (uint32_t)R, columns[T] = (uint32_t)C;
        df_res = (int64_t)L - 1 - (int64_t)R;
    }
};

}  // namespace

int model_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const uint32_t* kind, const uint32_t* labels,
                        const double* values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed, epik_amd_model_term* out,
                        epik_amd_model_info* info, double* stat, uint8_t* aliased, std::string& err, const uint32_t* strata)
{
    const size_t S = num_samples, T = num_terms, P = num_permutations;
    if (const int rc = model_arguments_valid(kind, labels, values, num_samples, num_terms, num_permutations, err); rc != EPIK_AMD_OK)
        return rc;
    const double na = na_value();
    // 1, 3 and 4: the complete cases with mass, the columns and the basis
    const design_basis basis(totals, S, kind, labels, values, T, aliased);
    const std::vector<size_t>& used = basis.used;
    const std::vector<std::vector<double>>& Q = basis.Q;
    const std::vector<uint32_t>&df = basis.df, &columns = basis.columns;
    const size_t L = used.size(), C = basis.C, R = Q.size();
    const int64_t df_res = basis.df_res;
    // 2: the Gower matrix, as pcoa_components_of_kr forms it
    std::vector<double> B(L * L, 0.0), r(L);
    for (size_t i = 0; i < L; ++i)
        for (size_t j = 0; j < L; ++j) {
            const double d = kr[used[i] * S + used[j]];
            B[i * L + j] = d * d;
        }
    double g = 0.0;
    for (size_t i = 0; i < L; ++i) {
        double acc = 0.0;
        for (size_t j = 0; j < L; ++j) acc = acc + B[j * L + i];  // (KR[u_j][u_i], the element the device's lanes read)
        r[i] = acc / (double)L;
        g = g + r[i];
    }
    if (L) g = g / (double)L;
    for (size_t i = 0; i < L; ++i)
        for (size_t j = i; j < L; ++j) B[i * L + j] = B[j * L + i] = -0.5 * (((B[i * L + j] - r[i]) - r[j]) + g);
    double ss_total = 0.0;
    for (size_t i = 0; i < L; ++i) ss_total = ss_total + B[i * L + i];
    // 5: SS_k of an arrangement into ss[T + 1], the model's last
    std::vector<double> tc(L);
    const auto sums = [&](const std::vector<uint32_t>& sigma, std::vector<double>& ss) {
        size_t c = 0;
        double model = 0.0;
        for (size_t t = 0; t < T; ++t) {
            double term = 0.0;
            for (uint32_t w = 0; w < df[t]; ++w, ++c) {
                const std::vector<double>& q = Q[c];
                double s = 0.0;
                for (size_t i = 0; i < L; ++i) {
                    double acc = 0.0;
                    const double* row = B.data() + i * L;
                    for (size_t j = 0; j < L; ++j) acc = acc + row[j] * q[sigma[j]];
                    s = s + q[sigma[i]] * acc;
                }
                term = term + s;
            }
            ss[t] = term;
            model = model + term;
        }
        ss[T] = model;
    };
    std::vector<uint32_t> sigma(L);
    for (size_t i = 0; i < L; ++i) sigma[i] = (uint32_t)i;
    std::vector<double> ss0(T + 1), ss(T + 1), f0(T + 1, na);
    sums(sigma, ss0);
    const double ss_res = ss_total - ss0[T];
    *info = epik_amd_model_info{(uint32_t)L, (uint32_t)T, (uint32_t)C, (uint32_t)R, df_res, ss_total, ss_res};
    const bool testable = df_res >= 1 && ss_res > 0.0;
    if (stat) std::fill(stat, stat + (T + 1) * (P + 1), na);
    for (size_t k = 0; k <= T; ++k) {
        out[k] = epik_amd_model_term{df[k], columns[k], 0, na, na, na, na};
        if (!df[k]) continue;
        out[k].ss = ss0[k];
        if (ss_total > 0.0) out[k].r2 = ss0[k] / ss_total;
        if (testable) out[k].f = f0[k] = (ss0[k] / (double)df[k]) / (ss_res / (double)df_res);
        if (testable && stat) stat[k * (P + 1)] = f0[k];
    }
    if (!testable || !R) return EPIK_AMD_OK;
    // 6 and 7: the permutations
    arrangements arrange(strata, L, [&](size_t i) { return used[i]; });
    for (uint32_t p = 1; p <= P; ++p) {
        sums(arrange.of(seed, p), ss);
        const double res = ss_total - ss[T];
        for (size_t k = 0; k <= T; ++k) {
            if (!df[k]) continue;
            const double f = res > 0.0 ? (ss[k] / (double)df[k]) / (res / (double)df_res) : HUGE_VAL;
            if (stat) stat[k * (P + 1) + p] = f;
            out[k].at_least += f >= f0[k];
        }
    }
    for (size_t k = 0; k <= T; ++k)
        if (df[k]) out[k].p = (double)(1 + out[k].at_least) / (double)(P + 1);
    return EPIK_AMD_OK;
}

int model_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                  const double* branch_length, const uint32_t* kind, const uint32_t* labels, const double* values, uint32_t num_terms,
                  uint32_t num_permutations, uint64_t seed, epik_amd_model_term* out, epik_amd_model_info* info, double* stat,
                  uint8_t* aliased, std::string& err, uint32_t metric, const uint32_t* strata)
{
    const size_t S = num_samples, N = num_branches;
    if (const int rc = model_arguments_valid(kind, labels, values, num_samples, num_terms, num_permutations, err); rc != EPIK_AMD_OK)
        return rc;
    std::vector<double> kr(S * S);
    if (const int rc = distance_matrix(mass, num_samples, num_branches, first, branch_length, metric, kr.data(), err); rc != EPIK_AMD_OK)
        return rc;
    std::vector<uint64_t> totals(S, 0);
    for (size_t s = 0; s < S; ++s)
        for (size_t b = 0; b < N; ++b) totals[s] += mass[s * N + b];
    return model_records_of_kr(kr.data(), totals.data(), num_samples, kind, labels, values, num_terms, num_permutations, seed, out, info,
                               stat, aliased, err, strata);
}

int edgemodel_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first, const uint32_t* kind,
                      const uint32_t* labels, const double* values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                      epik_amd_edgemodel* out, epik_amd_edgemodel_info* info, double* stat, double* max, uint8_t* aliased,
                      std::string& err, const uint32_t* strata)
{
    constexpr size_t F = EPIK_AMD_EDGEMODEL_FAMILIES;
    const size_t S = num_samples, N = num_branches, T = num_terms, P = num_permutations, row = P + 1;
    if (const int rc = model_arguments_valid(kind, labels, values, num_samples, num_terms, num_permutations, err); rc != EPIK_AMD_OK)
        return rc;
    kr_planes planes;
    if (const int rc = make_planes(mass, S, N, first, nullptr, planes, err); rc != EPIK_AMD_OK) return rc;
    const double na = na_value();
    const design_basis basis(planes.total.data(), S, kind, labels, values, T, aliased);
    const std::vector<size_t>& used = basis.used;
    const std::vector<uint32_t>& df = basis.df;
    const size_t L = used.size(), R = basis.Q.size();
    const int64_t df_res = basis.df_res;
    *info = epik_amd_edgemodel_info{(uint32_t)L, (uint32_t)T, (uint32_t)basis.C, (uint32_t)R, df_res, {}, {}};
    for (size_t k = 0; k < T; ++k) info->df[k] = df[k], info->term_columns[k] = basis.columns[k];
    const epik_amd_edgemodel_family none{na, na, na, na, na, na, 0, 0, 0, 0};
    for (size_t e = 0; e < T * N; ++e) out[e].family[0] = out[e].family[1] = none;
    if (stat) std::fill(stat, stat + T * F * N * row, na);
    if (max) std::fill(max, max + T * F * row, na);
    if (df_res < 1 || R == 0) return EPIK_AMD_OK;
    // the basis by position, a row a position: Qrow[i][c]; and the arranged rows of a chunk of permutations
    std::vector<double> Qrow(L * R);
    for (size_t c = 0; c < R; ++c)
        for (size_t i = 0; i < L; ++i) Qrow[i * R + c] = basis.Q[c][i];
    const size_t chunk = std::max<size_t>(1, ((size_t)8 << 20) / (L * R));
    std::vector<double> Qs(std::min(chunk, row) * L * R);
    arrangements arrange(strata, L, [&](size_t i) { return used[i]; });
    std::vector<double> mmax(T * F * row, 0.0), s(R), x[F];
    std::vector<char> any(F, 0);
    centred dev[F];
    // SS_k and phi_k of the sums s_c of one arrangement into ss[T] and phi[T] (phi means something where df_k >= 1); returns SS_res
    std::vector<double> phi(T), ss(T);
    const auto statistic = [&](double sxx) {
        size_t c = 0;
        double model = 0.0;
        for (size_t k = 0; k < T; ++k) {
            double term = 0.0;
            for (uint32_t w = 0; w < df[k]; ++w, ++c) term = term + s[c] * s[c];
            ss[k] = term;
            model = model + term;
        }
        const double res = sxx - model;
        for (size_t k = 0; k < T; ++k) phi[k] = res > 0.0 ? ss[k] / (ss[k] + res) : ss[k] > 0.0 ? 1.0 : 0.0;
        return res;
    };
    for (size_t p0 = 0; p0 < row; p0 += chunk) {
        const size_t np = std::min(chunk, row - p0);
        for (size_t k = 0; k < np; ++k) {
            double* q = Qs.data() + k * L * R;
            if (p0 + k == 0) {
                std::copy(Qrow.begin(), Qrow.end(), q);
                continue;
            }
            const std::vector<uint32_t>& sigma = arrange.of(seed, (uint32_t)(p0 + k));
            for (size_t i = 0; i < L; ++i) std::copy(Qrow.begin() + sigma[i] * R, Qrow.begin() + (sigma[i] + 1) * R, q + i * R);
        }
        for (size_t b = 0; b < N; ++b) {
            const bool inner = first[b] < b;
            branch_vectors(mass, planes, N, b, used, x[0], x[1]);
            for (size_t f = 0; f < (inner ? F : 1); ++f) {
                dev[f].of(x[f]);
                const double sxx = dev[f].ss;
                if (!(sxx > 0.0)) continue;
                const double* d = dev[f].d.data();
                for (size_t k = 0; k < np; ++k) {
                    const double* q = Qs.data() + k * L * R;
                    std::fill(s.begin(), s.end(), 0.0);
                    for (size_t i = 0; i < L; ++i)
                        for (size_t c = 0; c < R; ++c) s[c] = s[c] + q[i * R + c] * d[i];
                    const double res = statistic(sxx);
                    const size_t p = p0 + k;
                    for (size_t t = 0, c = 0; t < T; c += df[t], ++t) {
                        if (!df[t]) continue;
                        epik_amd_edgemodel_family& fam = out[t * N + b].family[f];
                        if (p == 0) {
                            fam = epik_amd_edgemodel_family{ss[t], ss[t] / sxx, phi[t], na, na, na, 0, 0, 0, 0};
                            if (res > 0.0) fam.f = (ss[t] / (double)df[t]) / (res / (double)df_res);
                            if (df[t] == 1) fam.sign = s[c] > 0.0 ? 1 : s[c] < 0.0 ? -1 : 0;
                            any[f] = 1;
                        }
                        const size_t cell = (t * F + f) * row + p;
                        if (stat) stat[((t * F + f) * N + b) * row + p] = phi[t];
                        if (phi[t] > mmax[cell]) mmax[cell] = phi[t];
                        fam.at_least += p >= 1 && phi[t] >= fam.partial_r2;
                    }
                }
            }
        }
    }
    // max_at_least by a search in the sorted maxima: a count, exact however it is found
    for (size_t t = 0; t < T; ++t)
        for (size_t f = 0; f < F; ++f) {
            if (!df[t] || !any[f]) continue;
            const double* m = mmax.data() + (t * F + f) * row;
            if (max) std::copy(m, m + row, max + (t * F + f) * row);
            std::vector<double> sorted(m + 1, m + row);
            std::sort(sorted.begin(), sorted.end());
            for (size_t b = 0; b < N; ++b) {
                epik_amd_edgemodel_family& fam = out[t * N + b].family[f];
                if (std::isnan(fam.partial_r2)) continue;
                fam.max_at_least = (uint64_t)(sorted.end() - std::lower_bound(sorted.begin(), sorted.end(), fam.partial_r2));
                fam.p = (double)(1 + fam.at_least) / (double)(P + 1);
                fam.p_adj = (double)(1 + fam.max_at_least) / (double)(P + 1);
            }
        }
    return EPIK_AMD_OK;
}

namespace {

int too_many_samples(uint32_t num_samples, const char* what, std::string& err)
{
    if (num_samples <= EPIK_AMD_MANTEL_MAX_SAMPLES) return EPIK_AMD_OK;
    err = std::string(what) + ": num_samples = " + std::to_string(num_samples) + " is above 8192, the most samples of this analysis";
    return EPIK_AMD_ERR_INVALID;
}

int permutations_in_range(uint32_t num_permutations, std::string& err)
{
    if (num_permutations >= 1 && num_permutations <= EPIK_AMD_PERMANOVA_MAX_PERMUTATIONS) return EPIK_AMD_OK;
    err = "num_permutations = " + std::to_string(num_permutations) + " is outside [1, 999999]";
    return EPIK_AMD_ERR_INVALID;
}

// the rule's triangle chain of f(i, j) over the pairs of n positions: the rows' chains, then the chain of the rows
template <class F>
double triangle_chain(size_t n, F f)
{
    double total = 0.0;
    for (size_t i = 0; i + 1 < n; ++i) {
        double t = 0.0;
        for (size_t j = i + 1; j < n; ++j) t = t + f(i, j);
        total = total + t;
    }
    return total;
}

// one of x, y, z over a list of n positions as a symmetric table (the diagonal is never read): the values of cell(i, j), i < j,
// or their midranks among the m of them; then the deviations from the chain's mean, and ss
struct mantel_table {
    std::vector<double> a;
    double ss = 0.0;
    template <class Cell>
    void fill(size_t n, Cell cell, bool ranks)
    {
        a.assign(n * n, 0.0);
        std::vector<double> v, r;
        std::vector<uint32_t> order;
        for (size_t i = 0; i < n; ++i)
            for (size_t j = i + 1; j < n; ++j) v.push_back(cell(i, j));
        if (ranks) midranks_sorted(v, order, r), v.swap(r);
        size_t e = 0;
        for (size_t i = 0; i < n; ++i)
            for (size_t j = i + 1; j < n; ++j) a[i * n + j] = a[j * n + i] = v[e++];
    }
    void centre(size_t n)
    {
        const double mean = triangle_chain(n, [&](size_t i, size_t j) { return a[i * n + j]; }) / (double)(n * (n - 1) / 2);
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < n; ++j)
                if (i != j) a[i * n + j] = a[i * n + j] - mean;
        ss = triangle_chain(n, [&](size_t i, size_t j) { return a[i * n + j] * a[i * n + j]; });
    }
};

// the rule's partial statistic; false where the radicand that moves with the permutation is not > 0
inline bool mantel_partial(double r_xy, double r_xz, double r_yz, double& stat)
{
    const double rad_x = 1.0 - r_xz * r_xz, rad_y = 1.0 - r_yz * r_yz;
    if (!(rad_x > 0.0) || !(rad_y > 0.0)) return false;
    stat = (r_xy - r_xz * r_yz) / (std::sqrt(rad_x) * std::sqrt(rad_y));
    return true;
}

}  // namespace

int mantel_arguments_valid(const mantel_sides& sides, uint32_t num_samples, uint32_t num_permutations, std::string& err)
{
    if (const int rc = too_many_samples(num_samples, "mantel", err); rc != EPIK_AMD_OK) return rc;
    const size_t S = num_samples, Mv = sides.num_columns, Mm = sides.num_matrices;
    if (Mv > EPIK_AMD_MANTEL_MAX_COLUMNS) {
        err = "num_columns = " + std::to_string(Mv) + " is outside [0, 64]";
        return EPIK_AMD_ERR_INVALID;
    }
    if (Mm > EPIK_AMD_MANTEL_MAX_MATRICES) {
        err = "num_matrices = " + std::to_string(Mm) + " is outside [0, 8]";
        return EPIK_AMD_ERR_INVALID;
    }
    if (Mv + Mm == 0) {
        err = "a Mantel test needs a side: num_columns and num_matrices are both 0";
        return EPIK_AMD_ERR_INVALID;
    }
    if ((Mv && !sides.values) || (Mm && (!sides.matrices || !sides.matrix_present))) {
        err = "null argument";
        return EPIK_AMD_ERR_INVALID;
    }
    if (sides.methods < 1 || sides.methods > (EPIK_AMD_MANTEL_PEARSON | EPIK_AMD_MANTEL_SPEARMAN)) {
        err = "methods = " + std::to_string(sides.methods) + " is outside [1, 3] (bit 0 pearson, bit 1 spearman)";
        return EPIK_AMD_ERR_INVALID;
    }
    if (sides.control != EPIK_AMD_MANTEL_NO_CONTROL && sides.control >= Mv + Mm) {
        err = "control = " + std::to_string(sides.control) + " names no side (there are " + std::to_string(Mv + Mm) + ")";
        return EPIK_AMD_ERR_INVALID;
    }
    if (const int rc = permutations_in_range(num_permutations, err); rc != EPIK_AMD_OK) return rc;
    for (size_t q = 0; q < Mv; ++q) {
        double least = HUGE_VAL, most = -HUGE_VAL;
        for (size_t s = 0; s < S; ++s) {
            const double v = sides.values[q * S + s];
            if (std::isinf(v)) {
                err = "sample " + std::to_string(s) + ", column " + std::to_string(q) + ": the value is infinite";
                return EPIK_AMD_ERR_INVALID;
            }
            if (v < least) least = v;
            if (v > most) most = v;
        }
        if (most > least && std::isinf(most - least)) {  // (|v_s - v_t| would be the +inf that pads the sort of the pairs)
            err = "column " + std::to_string(q) + ": the range of the values overflows a double";
            return EPIK_AMD_ERR_INVALID;
        }
    }
    for (size_t k = 0; k < Mm; ++k)
        for (size_t s = 0; s < S; ++s)
            for (size_t t = s + 1; t < S; ++t) {
                const double v = sides.matrices[(k * S + s) * S + t];
                if (!sides.matrix_present[k * S + s] || !sides.matrix_present[k * S + t] || (v >= 0.0 && std::isfinite(v))) continue;
                err = "matrix " + std::to_string(k) + ", cell [" + std::to_string(s) + "][" + std::to_string(t) +
                      "]: the distance is negative or not finite";
                return EPIK_AMD_ERR_INVALID;
            }
    return EPIK_AMD_OK;
}

int anosim_arguments_valid(const uint32_t* labels, uint32_t num_samples, uint32_t num_columns, uint32_t num_permutations, std::string& err)
{
    if (const int rc = too_many_samples(num_samples, "anosim", err); rc != EPIK_AMD_OK) return rc;
    return permanova_arguments_valid(labels, num_samples, num_columns, num_permutations, false, err);
}

int mantel_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const mantel_sides& sides,
                         uint32_t num_permutations, uint64_t seed, epik_amd_mantel* out, double* stat, std::string& err,
                         const uint32_t* strata)
{
    if (const int rc = mantel_arguments_valid(sides, num_samples, num_permutations, err); rc != EPIK_AMD_OK) return rc;
    const size_t S = num_samples, P = num_permutations, Mv = sides.num_columns, Q = sides.sides();
    const double na = na_value();
    if (stat) std::fill(stat, stat + (size_t)sides.tests() * (P + 1), na);
    const auto present = [&](size_t q, size_t s) {
        return q < Mv ? !std::isnan(sides.values[q * S + s]) : sides.matrix_present[(q - Mv) * S + s] != 0;
    };
    const auto distance = [&](size_t q, size_t s, size_t t) {  // (s < t)
        return q < Mv ? std::fabs(sides.values[q * S + s] - sides.values[q * S + t]) : sides.matrices[((q - Mv) * S + s) * S + t];
    };
    size_t test = 0;
    for (size_t q = 0; q < Q; ++q)
        for (uint32_t method = 0; method < 2; ++method) {
            if (!(sides.methods >> method & 1u)) continue;
            const bool partial = sides.control != EPIK_AMD_MANTEL_NO_CONTROL && sides.control != q;
            const size_t z_side = sides.control;
            std::vector<uint32_t> u;
            for (size_t s = 0; s < S; ++s)
                if (totals[s] != 0 && present(q, s) && (!partial || present(z_side, s))) u.push_back((uint32_t)s);
            const size_t n = u.size();
            epik_amd_mantel& rec = out[test];
            double* row = stat ? stat + test * (P + 1) : nullptr;
            ++test;
            rec = epik_amd_mantel{(uint32_t)n, (uint32_t)q, method, partial ? 1u : 0u, 0, na, na, na, na, na};
            if (n < 3) continue;
            mantel_table x, y, z;
            x.fill(n, [&](size_t i, size_t j) { return kr[(size_t)u[i] * S + u[j]]; }, method == 1), x.centre(n);
            y.fill(n, [&](size_t i, size_t j) { return distance(q, u[i], u[j]); }, method == 1), y.centre(n);
            if (partial) z.fill(n, [&](size_t i, size_t j) { return distance(z_side, u[i], u[j]); }, method == 1), z.centre(n);
            if (x.ss == 0.0 || y.ss == 0.0 || (partial && z.ss == 0.0)) continue;
            const auto product = [&](const mantel_table& a, const mantel_table& b) {
                return triangle_chain(n, [&](size_t i, size_t j) { return a.a[i * n + j] * b.a[i * n + j]; });
            };
            const double den_xy = std::sqrt(x.ss * y.ss), r_xy = product(x, y) / den_xy;
            double den_xz = 0.0, r_xz = na, r_yz = na, stat0 = r_xy;
            if (partial) {
                den_xz = std::sqrt(x.ss * z.ss);
                r_xz = product(x, z) / den_xz, r_yz = product(y, z) / std::sqrt(y.ss * z.ss);
                if (!mantel_partial(r_xy, r_xz, r_yz, stat0)) continue;
            }
            rec.r = r_xy, rec.r_xz = r_xz, rec.r_yz = r_yz, rec.stat = stat0;
            if (row) row[0] = stat0;
            arrangements arrange(strata, n, [&](size_t i) { return u[i]; });
            uint64_t at_least = 0;
            for (uint32_t p = 1; p <= P; ++p) {
                const std::vector<uint32_t>& sigma = arrange.of(seed, p);
                const auto permuted = [&](const mantel_table& b) {
                    return triangle_chain(n, [&](size_t i, size_t j) { return x.a[(size_t)sigma[i] * n + sigma[j]] * b.a[i * n + j]; });
                };
                double value = permuted(y) / den_xy;
                if (partial && !mantel_partial(value, permuted(z) / den_xz, r_yz, value)) continue;  // (the row keeps its NA)
                if (row) row[p] = value;
                at_least += value >= stat0;
            }
            rec.at_least = at_least;
            rec.p = (double)(1 + at_least) / (double)(P + 1);
        }
    return EPIK_AMD_OK;
}

namespace {

// the matrix of `metric` and T_s from the cells: what the _host entries of the distance tests start from
int matrix_and_totals(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                      const double* branch_length, uint32_t metric, std::vector<double>& kr, std::vector<uint64_t>& totals,
                      std::string& err)
{
    const size_t S = num_samples, N = num_branches;
    kr.resize(S * S), totals.assign(S, 0);
    if (const int rc = distance_matrix(mass, num_samples, num_branches, first, branch_length, metric, kr.data(), err); rc != EPIK_AMD_OK)
        return rc;
    for (size_t s = 0; s < S; ++s)
        for (size_t b = 0; b < N; ++b) totals[s] += mass[s * N + b];
    return EPIK_AMD_OK;
}

}  // namespace

int mantel_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                   const double* branch_length, const mantel_sides& sides, uint32_t num_permutations, uint64_t seed,
                   epik_amd_mantel* out, double* stat, std::string& err, uint32_t metric, const uint32_t* strata)
{
    if (const int rc = mantel_arguments_valid(sides, num_samples, num_permutations, err); rc != EPIK_AMD_OK) return rc;
    std::vector<double> kr;
    std::vector<uint64_t> totals;
    if (const int rc = matrix_and_totals(mass, num_samples, num_branches, first, branch_length, metric, kr, totals, err); rc != EPIK_AMD_OK)
        return rc;
    return mantel_records_of_kr(kr.data(), totals.data(), num_samples, sides, num_permutations, seed, out, stat, err, strata);
}

int anosim_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const uint32_t* labels,
                         uint32_t num_columns, uint32_t num_permutations, uint64_t seed, epik_amd_anosim* out, double* stat,
                         std::string& err, const uint32_t* strata)
{
    if (const int rc = anosim_arguments_valid(labels, num_samples, num_columns, num_permutations, err); rc != EPIK_AMD_OK) return rc;
    const size_t S = num_samples, M = num_columns, P = num_permutations;
    const double na = na_value();
    if (stat) std::fill(stat, stat + M * (P + 1), na);
    for (size_t c = 0; c < M; ++c) {
        std::vector<uint32_t> idx, lam, size, group_of(EPIK_AMD_PERMANOVA_MAX_GROUPS, EPIK_AMD_PERMANOVA_MISSING);
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (totals[s] == 0 || v == EPIK_AMD_PERMANOVA_MISSING) continue;
            if (group_of[v] == EPIK_AMD_PERMANOVA_MISSING) group_of[v] = (uint32_t)size.size(), size.push_back(0);
            idx.push_back((uint32_t)s), lam.push_back(group_of[v]), ++size[group_of[v]];
        }
        const size_t n = idx.size(), G = size.size();
        out[c] = epik_amd_anosim{(uint32_t)n, (uint32_t)G, 0, na, na, na, na};
        const uint64_t m = (uint64_t)n * (n ? n - 1 : 0) / 2;
        uint64_t m_within = 0;
        for (size_t g = 0; g < G; ++g) m_within += (uint64_t)size[g] * (size[g] - 1) / 2;
        if (G < 2 || m_within < 1) continue;
        mantel_table x;
        x.fill(n, [&](size_t i, size_t j) { return kr[(size_t)idx[i] * S + idx[j]]; }, true);
        const double all = (double)(m * (m + 1) / 2), half = (double)m / 2.0;
        double between = 0.0, within = 0.0;
        const auto statistic = [&](const std::vector<uint32_t>& mu) {
            double w = 0.0;
            for (size_t i = 0; i < n; ++i)
                for (size_t j = i + 1; j < n; ++j)
                    if (mu[i] == mu[j]) w = w + x.a[i * n + j];
            within = w / (double)m_within, between = (all - w) / (double)(m - m_within);
            return (between - within) / half;
        };
        const double r0 = statistic(lam);
        out[c].r = r0, out[c].mean_between = between, out[c].mean_within = within;
        double* row = stat ? stat + c * (P + 1) : nullptr;
        if (row) row[0] = r0;
        arrangements arrange(strata, n, [&](size_t i) { return idx[i]; });
        std::vector<uint32_t> mu(n);
        uint64_t at_least = 0;
        for (uint32_t p = 1; p <= P; ++p) {
            const std::vector<uint32_t>& sigma = arrange.of(seed, p);
            for (size_t i = 0; i < n; ++i) mu[i] = lam[sigma[i]];
            const double value = statistic(mu);
            if (row) row[p] = value;
            at_least += value >= r0;
        }
        out[c].at_least = at_least;
        out[c].p = (double)(1 + at_least) / (double)(P + 1);
    }
    return EPIK_AMD_OK;
}

int anosim_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                   const double* branch_length, const uint32_t* labels, uint32_t num_columns, uint32_t num_permutations,
                   uint64_t seed, epik_amd_anosim* out, double* stat, std::string& err, uint32_t metric, const uint32_t* strata)
{
    if (const int rc = anosim_arguments_valid(labels, num_samples, num_columns, num_permutations, err); rc != EPIK_AMD_OK) return rc;
    std::vector<double> kr;
    std::vector<uint64_t> totals;
    if (const int rc = matrix_and_totals(mass, num_samples, num_branches, first, branch_length, metric, kr, totals, err); rc != EPIK_AMD_OK)
        return rc;
    return anosim_records_of_kr(kr.data(), totals.data(), num_samples, labels, num_columns, num_permutations, seed, out, stat, err,
                                strata);
}

cohort_factors read_cohort_factors(const std::string& file, const std::vector<cohort_sample>& samples, bool pairwise, size_t most_labels,
                                   const char* flag)
{
    std::ifstream in(file);
    if (!in) throw std::runtime_error(std::string(flag) + ": cannot open the factor file " + file);
    std::map<std::string, size_t> index;
    for (size_t s = 0; s < samples.size(); ++s) index[samples[s].name] = s;
    cohort_factors factors;
    std::vector<size_t> seen(samples.size(), 0);  // the line that gave the sample, 0: none yet
    std::vector<std::map<std::string, uint32_t>> id_of;
    bool have_header = false;
    std::string line;
    for (size_t number = 1; std::getline(in, line); ++number) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::string where = std::string(flag) + ": " + file + " line " + std::to_string(number);
        const auto fields = split_tabs(line);
        if (!have_header) {
            if (fields[0] != "sample") throw std::runtime_error(where + ": the header must begin with 'sample'");
            if (fields.size() < 2 || fields.size() > 1 + EPIK_AMD_PERMANOVA_MAX_COLUMNS)
                throw std::runtime_error(where + ": the header names " + std::to_string(fields.size() - 1) + " columns, not 1 to 64");
            std::set<std::string> names;
            for (size_t c = 1; c < fields.size(); ++c) {
                if (fields[c].empty()) throw std::runtime_error(where + ": column " + std::to_string(c) + " has an empty name");
                if (!names.insert(fields[c]).second)
                    throw std::runtime_error(where + ": the column name '" + fields[c] + "' is given twice");
                factors.columns.push_back(fields[c]);
            }
            factors.labels.assign(samples.size() * factors.columns.size(), EPIK_AMD_PERMANOVA_MISSING);
            factors.names.resize(factors.columns.size()), id_of.resize(factors.columns.size());
            have_header = true;
            continue;
        }
        const size_t M = factors.columns.size();
        if (fields.size() != M + 1)
            throw std::runtime_error(where + ": " + std::to_string(fields.size()) + " fields, not " + std::to_string(M + 1));
        const auto found = index.find(fields[0]);
        if (found == index.end()) {
            ++factors.skipped;
            continue;
        }
        const size_t s = found->second;
        if (seen[s])
            throw std::runtime_error(where + ": the sample '" + fields[0] + "' is given twice (first on line " +
                                     std::to_string(seen[s]) + ")");
        seen[s] = number;
        for (size_t c = 0; c < M; ++c) {
            const std::string& v = fields[c + 1];
            if (v.empty() || v == "NA") continue;
            const auto [it, fresh] = id_of[c].emplace(v, (uint32_t)factors.names[c].size());
            if (fresh) {
                const size_t most = most_labels ? most_labels : pairwise ? EPIK_AMD_PERMANOVA_MAX_PAIR_GROUPS : EPIK_AMD_PERMANOVA_MAX_GROUPS;
                if (factors.names[c].size() == most)
                    throw std::runtime_error(where + ", column " + factors.columns[c] + ": '" + v + "' is label number " +
                                             std::to_string(most + 1) + ", more than " + std::to_string(most) +
                                             (pairwise && !most_labels ? " (the most of --cohort-permanova-pairwise)" : ""));
                factors.names[c].push_back(v);
            }
            factors.labels[s * M + c] = it->second;
        }
    }
    if (!have_header) throw std::runtime_error(std::string(flag) + ": " + file + " has no header line");
    for (size_t s = 0; s < samples.size(); ++s)
        if (!seen[s]) throw std::runtime_error(std::string(flag) + ": " + file + " has no line for the sample '" + samples[s].name + "'");
    return factors;
}

cohort_design read_cohort_design(const std::string& file, const std::string& terms, const std::vector<cohort_sample>& samples)
{
    const std::string flag = "--cohort-model";
    cohort_design design;
    // the terms: f:NAME or n:NAME, comma-separated, in test order
    for (size_t at = 0; at <= terms.size();) {
        const size_t comma = std::min(terms.find(',', at), terms.size());
        const std::string term = terms.substr(at, comma - at);
        at = comma + 1;
        const std::string where = "--cohort-model-terms: term " + std::to_string(design.terms.size() + 1) + " ('" + term + "')";
        if (term.size() < 3 || term[1] != ':' || (term[0] != 'f' && term[0] != 'n'))
            throw std::runtime_error(where + " is not f:NAME (a factor) or n:NAME (numeric)");
        const std::string name = term.substr(2);
        if (std::find(design.terms.begin(), design.terms.end(), name) != design.terms.end())
            throw std::runtime_error(where + ": the column '" + name + "' is given twice");
        if (design.terms.size() == EPIK_AMD_MODEL_MAX_TERMS) throw std::runtime_error("--cohort-model-terms: more than 16 terms");
        design.terms.push_back(name), design.kind.push_back(term[0] == 'n');
    }
    const size_t T = design.terms.size();
    std::ifstream in(file);
    if (!in) throw std::runtime_error(flag + ": cannot open the design file " + file);
    std::map<std::string, size_t> index;
    for (size_t s = 0; s < samples.size(); ++s) index[samples[s].name] = s;
    design.names.resize(T);
    design.labels.assign(samples.size() * T, EPIK_AMD_MODEL_MISSING);
    design.values.assign(samples.size() * T, std::nan(""));
    std::vector<size_t> seen(samples.size(), 0), field_of(T, 0);  // the line that gave the sample; the field of a term
    std::vector<std::map<std::string, uint32_t>> id_of(T);
    size_t fields_a_line = 0;
    std::string line;
    for (size_t number = 1; std::getline(in, line); ++number) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::string where = flag + ": " + file + " line " + std::to_string(number);
        const auto fields = split_tabs(line);
        if (!fields_a_line) {
            if (fields[0] != "sample") throw std::runtime_error(where + ": the header must begin with 'sample'");
            if (fields.size() < 2) throw std::runtime_error(where + ": the header names no column");
            std::set<std::string> names;
            for (size_t c = 1; c < fields.size(); ++c) {
                if (fields[c].empty()) throw std::runtime_error(where + ": column " + std::to_string(c) + " has an empty name");
                if (!names.insert(fields[c]).second)
                    throw std::runtime_error(where + ": the column name '" + fields[c] + "' is given twice");
            }
            for (size_t t = 0; t < T; ++t) {
                const auto found = std::find(fields.begin() + 1, fields.end(), design.terms[t]);
                if (found == fields.end())
                    throw std::runtime_error(where + ": the header has no column '" + design.terms[t] + "' (term " + std::to_string(t + 1) +
                                             " of --cohort-model-terms)");
                field_of[t] = (size_t)(found - fields.begin());
            }
            fields_a_line = fields.size();
            continue;
        }
        if (fields.size() != fields_a_line)
            throw std::runtime_error(where + ": " + std::to_string(fields.size()) + " fields, not " + std::to_string(fields_a_line));
        const auto found = index.find(fields[0]);
        if (found == index.end()) {
            ++design.skipped;
            continue;
        }
        const size_t s = found->second;
        if (seen[s])
            throw std::runtime_error(where + ": the sample '" + fields[0] + "' is given twice (first on line " +
                                     std::to_string(seen[s]) + ")");
        seen[s] = number;
        for (size_t t = 0; t < T; ++t) {
            const std::string& v = fields[field_of[t]];
            if (v.empty() || v == "NA") continue;
            const std::string at = where + ", column " + design.terms[t] + ": ";
            if (design.kind[t]) {
                if (!is_number(v)) throw std::runtime_error(at + "'" + v + "' is not a number, empty or NA");
                const double value = std::strtod(v.c_str(), nullptr);
                if (std::isinf(value)) throw std::runtime_error(at + "'" + v + "' overflows a double");
                design.values[s * T + t] = value;
                continue;
            }
            const auto [it, fresh] = id_of[t].emplace(v, (uint32_t)design.names[t].size());
            if (fresh) {
                if (design.names[t].size() == EPIK_AMD_MODEL_MAX_GROUPS)
                    throw std::runtime_error(at + "'" + v + "' is label number 33, more than 32");
                design.names[t].push_back(v);
            }
            design.labels[s * T + t] = it->second;
        }
    }
    if (!fields_a_line) throw std::runtime_error(flag + ": " + file + " has no header line");
    for (size_t s = 0; s < samples.size(); ++s)
        if (!seen[s]) throw std::runtime_error(flag + ": " + file + " has no line for the sample '" + samples[s].name + "'");
    return design;
}

std::vector<cohort_sample> read_cohort_list(const std::string& list_file)
{
    std::ifstream in(list_file);
    if (!in) throw std::runtime_error("--cohort: cannot open the list of samples " + list_file);
    const auto slash = list_file.find_last_of('/');
    const std::string dir = slash == std::string::npos ? std::string() : list_file.substr(0, slash + 1);
    std::vector<cohort_sample> samples;
    std::set<std::string> names;
    std::string line;
    for (size_t number = 1; std::getline(in, line); ++number) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::string where = "--cohort: " + list_file + " line " + std::to_string(number) + ": ";
        const auto tab = line.find('\t');
        if (tab == std::string::npos) throw std::runtime_error(where + "not a name<TAB>path line");
        cohort_sample sample{line.substr(0, tab), line.substr(tab + 1)};
        if (sample.name.empty() || sample.path.empty() || sample.path.find('\t') != std::string::npos)
            throw std::runtime_error(where + "not a name<TAB>path line");
        if (!names.insert(sample.name).second) throw std::runtime_error(where + "the name '" + sample.name + "' is given twice");
        if (sample.path[0] != '/') sample.path = dir + sample.path;
        if (!std::ifstream(sample.path)) throw std::runtime_error(where + "cannot read " + sample.path);
        samples.push_back(std::move(sample));
    }
    if (samples.empty()) throw std::runtime_error("--cohort: " + list_file + " names no sample");
    return samples;
}

std::string make_cohort_filename(const std::string& what, const std::string& list_file, const std::string& output_dir,
                                 const std::string& extension)
{
    const auto slash = list_file.find_last_of('/');
    const std::string base = slash == std::string::npos ? list_file : list_file.substr(slash + 1);
    std::string dir = output_dir;
    if (!dir.empty() && dir.back() != '/') dir.push_back('/');
    return dir + "cohort_" + what + "_" + base + extension;
}

std::string format_cohort_samples_tsv(const std::vector<cohort_sample>& samples, const sample_cohort& cohort)
{
    std::string out = "name\trecords\tplaced\tno_hit\ttoo_short\ttoo_narrow\ttotal_mass_q\n";
    for (size_t s = 0; s < samples.size(); ++s) {
        const auto& t = cohort.totals[s];
        uint64_t total = 0;
        for (size_t b = 0; b < cohort.num_branches; ++b) total += cohort.mass[s * cohort.num_branches + b];
        out += samples[s].name + '\t' + std::to_string(t.placed + t.no_hit + t.too_short + t.too_narrow) + '\t' +
               std::to_string(t.placed) + '\t' + std::to_string(t.no_hit) + '\t' + std::to_string(t.too_short) + '\t' +
               std::to_string(t.too_narrow) + '\t' + std::to_string(total) + '\n';
    }
    return out;
}

std::string format_cohort_profile_tsv(const std::vector<cohort_sample>& samples, const sample_cohort& cohort)
{
    std::string out = "name\tedge_num\tbest\tmass_q\n";
    for (size_t s = 0; s < samples.size(); ++s)
        for (size_t b = 0; b < cohort.num_branches; ++b) {
            const uint64_t m = cohort.mass[s * cohort.num_branches + b], best = cohort.best[s * cohort.num_branches + b];
            if (m == 0 && best == 0) continue;
            out += samples[s].name + '\t' + std::to_string(b) + '\t' + std::to_string(best) + '\t' + std::to_string(m) + '\n';
        }
    return out;
}

const char* distance_name(uint32_t metric)
{
    static const char* const names[] = {"kr", "unweighted", "weighted", "generalized"};
    if (metric > EPIK_AMD_DISTANCE_GENERALIZED) throw std::runtime_error("metric = " + std::to_string(metric) + " is no distance");
    return names[metric];
}

uint32_t distance_of_name(const std::string& name, bool with_kr)
{
    for (uint32_t metric = with_kr ? EPIK_AMD_DISTANCE_KR : EPIK_AMD_DISTANCE_UNWEIGHTED; metric <= EPIK_AMD_DISTANCE_GENERALIZED; ++metric)
        if (name == distance_name(metric)) return metric;
    return 0xffffffffu;
}

std::vector<uint32_t> parse_unifrac_list(const std::string& list)
{
    std::vector<uint32_t> metrics;
    if (list == "all") return {EPIK_AMD_DISTANCE_UNWEIGHTED, EPIK_AMD_DISTANCE_WEIGHTED, EPIK_AMD_DISTANCE_GENERALIZED};
    for (size_t at = 0; at <= list.size();) {
        const size_t comma = std::min(list.find(',', at), list.size());
        const std::string name = list.substr(at, comma - at);
        const uint32_t metric = distance_of_name(name, false);
        if (metric == 0xffffffffu)
            throw std::runtime_error("--cohort-unifrac: '" + name + "' is no UniFrac distance (unweighted, weighted, generalized, or all)");
        if (std::find(metrics.begin(), metrics.end(), metric) != metrics.end())
            throw std::runtime_error("--cohort-unifrac: '" + name + "' is given twice");
        metrics.push_back(metric);
        at = comma + 1;
    }
    return metrics;
}

std::string distance_field(uint32_t metric)
{
    return metric == EPIK_AMD_DISTANCE_KR ? std::string() : std::string("\tdistance=") + distance_name(metric);
}

std::string format_cohort_kr_tsv(const std::vector<cohort_sample>& samples, const std::vector<double>& kr)
{
    const size_t S = samples.size();
    std::string out = "name";
    for (const auto& sample : samples) out += '\t' + sample.name;
    out += '\n';
    char text[40];
    for (size_t s = 0; s < S; ++s) {
        out += samples[s].name;
        for (size_t t = 0; t < S; ++t) {
            std::snprintf(text, sizeof text, "%.17g", kr[s * S + t]);
            out += '\t';
            out += text;
        }
        out += '\n';
    }
    return out;
}

namespace {

std::string g17(double v)
{
    char text[40];
    std::snprintf(text, sizeof text, "%.17g", v);
    return text;
}

// a sample's name as a newick label: as it is when every character is of [A-Za-z0-9_.-], else '...', inner quotes doubled
std::string newick_label(const std::string& name)
{
    bool plain = !name.empty();
    for (const char ch : name)
        plain = plain && ((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '.' || ch == '-');
    if (plain) return name;
    std::string out = "'";
    for (const char ch : name) {
        if (ch == '\'') out += '\'';
        out += ch;
    }
    return out + "'";
}

}  // namespace

std::string format_squash_tsv(const std::vector<cohort_sample>& samples, const std::vector<char>& live,
                              const epik_amd_squash_merge* merges, uint32_t num_merges)
{
    const size_t S = samples.size();
    size_t clustered = 0;
    for (size_t s = 0; s < S; ++s) clustered += live[s] ? 1 : 0;
    std::string out = "# epik_amd squash v1  samples=" + std::to_string(S) + " clustered=" + std::to_string(clustered) +
                      " merges=" + std::to_string(num_merges) + "\n";
    for (size_t s = 0; s < S; ++s)
        if (!live[s]) out += "# unclustered\t" + samples[s].name + "\n";
    out += "step\tnode\ta\tb\tsize\tdist\tlen_a\tlen_b\n";
    std::vector<uint64_t> size(S + num_merges, 1);
    for (uint32_t t = 0; t < num_merges; ++t) {
        size[S + t] = size.at(merges[t].a) + size.at(merges[t].b);
        out += std::to_string(t) + '\t' + std::to_string(S + t) + '\t' + std::to_string(merges[t].a) + '\t' +
               std::to_string(merges[t].b) + '\t' + std::to_string(size[S + t]) + '\t' + g17(merges[t].dist) + '\t' +
               g17(merges[t].len_a) + '\t' + g17(merges[t].len_b) + '\n';
    }
    return out;
}

std::string format_squash_newick(const std::vector<cohort_sample>& samples, const std::vector<char>& live,
                                 const epik_amd_squash_merge* merges, uint32_t num_merges)
{
    const size_t S = samples.size();
    std::vector<std::string> text(S + num_merges);  // (bottom up: a record names only nodes made before it)
    for (size_t s = 0; s < S; ++s)
        if (live[s]) text[s] = newick_label(samples[s].name);
    for (uint32_t t = 0; t < num_merges; ++t)
        text[S + t] = "(" + std::move(text.at(merges[t].a)) + ":" + g17(merges[t].len_a) + "," + std::move(text.at(merges[t].b)) +
                      ":" + g17(merges[t].len_b) + ")";
    if (num_merges) return text[S + num_merges - 1] + ";\n";
    for (size_t s = 0; s < S; ++s)
        if (live[s]) return text[s] + ";\n";
    return ";\n";
}

std::string format_epca_tsv(const std::vector<cohort_sample>& samples, const std::vector<char>& used, uint32_t num_components,
                            const double* mu, const double* proj, const epik_amd_epca_info& info)
{
    const size_t S = samples.size(), K = num_components, Kc = info.components;
    std::string out = "# epik_amd epca v1  samples=" + std::to_string(S) + " used=" + std::to_string(info.used) +
                      " components=" + std::to_string(Kc) + " sweeps=" + std::to_string(info.sweeps) +
                      " converged=" + std::to_string(info.converged) + "\n";
    for (size_t s = 0; s < S; ++s)
        if (!used[s]) out += "# unused\t" + samples[s].name + "\n";
    const double floor_mu = std::ldexp(1.0, -40) * info.scale, denominator = (double)std::max<uint32_t>(info.used, 2) - 1.0;
    for (size_t k = 0; k < Kc; ++k)
        out += "# component\t" + std::to_string(k + 1) + '\t' + g17(mu[k]) + '\t' + g17(mu[k] / denominator) + '\t' +
               g17(info.trace != 0.0 ? mu[k] / info.trace : 0.0) + '\t' + (mu[k] > floor_mu ? "ok" : "null") + '\n';
    out += "name";
    for (size_t k = 0; k < Kc; ++k) out += "\tpc" + std::to_string(k + 1);
    out += '\n';
    for (size_t s = 0; s < S; ++s) {
        if (!used[s]) continue;
        out += samples[s].name;
        for (size_t k = 0; k < Kc; ++k) out += '\t' + g17(proj[s * K + k]);
        out += '\n';
    }
    return out;
}

std::string format_epca_edges_tsv(const std::vector<uint32_t>& first, const double* edge, const epik_amd_epca_info& info)
{
    const size_t N = first.size(), Kc = info.components;
    std::string out = "edge_num";
    for (size_t k = 0; k < Kc; ++k) out += "\tpc" + std::to_string(k + 1);
    out += '\n';
    for (size_t b = 0; b < N; ++b) {
        if (!(first[b] < b)) continue;
        out += std::to_string(b);
        for (size_t k = 0; k < Kc; ++k) out += '\t' + g17(edge[k * N + b]);
        out += '\n';
    }
    return out;
}

std::string format_pcoa_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals, uint32_t num_components,
                            const double* mu, const double* coord, const epik_amd_pcoa_info& info, uint32_t distance)
{
    const size_t S = samples.size(), K = num_components, Kc = info.components, L = info.used;
    const double floor_mu = std::ldexp(1.0, -40) * info.scale;
    std::string out = "# epik_amd pcoa v1  samples=" + std::to_string(S) + " used=" + std::to_string(L) +
                      " components=" + std::to_string(Kc) + " sweeps=" + std::to_string(info.sweeps) +
                      " converged=" + std::to_string(info.converged) +
                      " negative=" + g17(info.pos != 0.0 ? (0.0 - info.neg) / info.pos : 0.0) + distance_field(distance) + "\n";
    for (size_t s = 0; s < S; ++s)
        if (totals[s] == 0) out += "# unused\t" + samples[s].name + "\n";
    for (size_t k = 0; k < L; ++k)
        out += "# eigenvalue\t" + std::to_string(k + 1) + '\t' + g17(mu[k]) + '\t' + g17(info.pos != 0.0 ? mu[k] / info.pos : 0.0) +
               '\t' + (mu[k] > floor_mu ? "real" : mu[k] < -floor_mu ? "negative" : "null") + '\n';
    out += "name";
    for (size_t k = 0; k < Kc; ++k) out += "\tpc" + std::to_string(k + 1);
    out += '\n';
    for (size_t s = 0; s < S; ++s) {
        if (totals[s] == 0) continue;
        out += samples[s].name;
        for (size_t k = 0; k < Kc; ++k) out += '\t' + g17(coord[s * K + k]);
        out += '\n';
    }
    return out;
}

std::string format_kmeans_tsv(const std::vector<cohort_sample>& samples, const epik_amd_kmeans_sample* records,
                              const epik_amd_kmeans_cluster* clusters, const epik_amd_kmeans_info& info)
{
    const size_t S = samples.size();
    std::string out = "# epik_amd kmeans v1  samples=" + std::to_string(S) + " used=" + std::to_string(info.used) +
                      " clusters=" + std::to_string(info.clusters) + " iterations=" + std::to_string(info.iterations) +
                      " converged=" + std::to_string(info.converged) + "\n";
    for (size_t s = 0; s < S; ++s)
        if (records[s].cluster == EPIK_AMD_KMEANS_NONE) out += "# unused\t" + samples[s].name + "\n";
    for (size_t k = 0; k < info.clusters; ++k)
        out += "# cluster\t" + std::to_string(k) + '\t' + std::to_string(clusters[k].size) + '\t' + samples.at(clusters[k].seed).name +
               '\t' + g17(clusters[k].sum_dist) + '\t' + g17(clusters[k].sum_sq) + '\n';
    out += "name\tcluster\tdist\n";
    for (size_t s = 0; s < S; ++s)
        if (records[s].cluster != EPIK_AMD_KMEANS_NONE)
            out += samples[s].name + '\t' + std::to_string(records[s].cluster) + '\t' + g17(records[s].dist) + '\n';
    return out;
}

std::string format_kmeans_centroids_tsv(const double* centroids, uint32_t num_branches, const epik_amd_kmeans_info& info)
{
    const size_t N = num_branches;
    std::string out = "cluster\tedge_num\tmass\n";
    for (size_t k = 0; k < info.clusters; ++k)
        for (size_t b = 0; b < N; ++b)
            if (centroids[k * N + b] != 0.0) out += std::to_string(k) + '\t' + std::to_string(b) + '\t' + g17(centroids[k * N + b]) + '\n';
    return out;
}

std::string format_alpha_tsv(const std::vector<cohort_sample>& samples, const epik_amd_alpha* alpha)
{
    const size_t S = samples.size();
    size_t used = 0;
    for (size_t s = 0; s < S; ++s) used += alpha[s].pd != -1.0;
    std::string out = "# epik_amd alpha v1  samples=" + std::to_string(S) + " used=" + std::to_string(used) + "\n";
    for (size_t s = 0; s < S; ++s)
        if (alpha[s].pd == -1.0) out += "# unused\t" + samples[s].name + "\n";
    out += "name\tpd\trooted_pd\tbwpd_0.5\tbwpd_1\tquadratic_entropy\n";
    for (size_t s = 0; s < S; ++s)
        if (alpha[s].pd != -1.0)
            out += samples[s].name + '\t' + g17(alpha[s].pd) + '\t' + g17(alpha[s].rooted_pd) + '\t' + g17(alpha[s].bwpd_half) + '\t' +
                   g17(alpha[s].bwpd_one) + '\t' + g17(alpha[s].quadratic) + '\n';
    return out;
}

std::string format_rarefy_tsv(const std::vector<cohort_sample>& samples, const uint64_t* reads, uint32_t depth_step,
                              uint32_t num_depths, const double* curve)
{
    const size_t S = samples.size(), J = num_depths;
    const auto rarefiable = [&](size_t s) { return reads[s] != 0 && reads[s] < (1ull << 53); };
    size_t used = 0;
    for (size_t s = 0; s < S; ++s) used += rarefiable(s);
    std::string out = "# epik_amd rarefy v1  samples=" + std::to_string(S) + " used=" + std::to_string(used) +
                      " step=" + std::to_string(depth_step) + " depths=" + std::to_string(J) + "\n";
    for (size_t s = 0; s < S; ++s)
        if (!rarefiable(s)) out += "# unused\t" + samples[s].name + "\n";
    out += "name\tk\treads\tpd\trooted_pd\n";
    for (size_t s = 0; s < S; ++s) {
        if (!rarefiable(s)) continue;
        for (size_t j = 0; j < J && (uint64_t)(j + 1) * depth_step <= reads[s]; ++j)
            out += samples[s].name + '\t' + std::to_string((uint64_t)(j + 1) * depth_step) + '\t' + std::to_string(reads[s]) + '\t' +
                   g17(curve[(s * J + j) * 2]) + '\t' + g17(curve[(s * J + j) * 2 + 1]) + '\n';
    }
    return out;
}

namespace {

std::string g17_or_na(double v) { return std::isnan(v) ? std::string("NA") : g17(v); }

// the first line of a file over the used samples (T_s > 0), then a "# unused" line per sample without mass
std::string used_head(const std::vector<cohort_sample>& samples, const uint64_t* totals, const char* what, const std::string& more)
{
    size_t used = 0;
    std::string unused;
    for (size_t s = 0; s < samples.size(); ++s) {
        if (totals[s] != 0)
            ++used;
        else
            unused += "# unused\t" + samples[s].name + "\n";
    }
    return "# epik_amd " + std::string(what) + " v1  samples=" + std::to_string(samples.size()) + " used=" + std::to_string(used) +
           more + "\n" + unused;
}

}  // namespace

std::string format_correlation_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                                   const std::vector<std::string>& columns, uint32_t num_branches,
                                   const epik_amd_correlation* records, const uint32_t* used_of)
{
    const size_t N = num_branches, M = columns.size();
    std::string out = used_head(samples, totals, "correlation", " columns=" + std::to_string(M));
    for (size_t c = 0; c < M; ++c) out += "# column\t" + std::to_string(c) + '\t' + columns[c] + '\t' + std::to_string(used_of[c]) + '\n';
    out += "edge_num\tcolumn\tmass_pearson\tmass_spearman\timbalance_pearson\timbalance_spearman\n";
    for (size_t b = 0; b < N; ++b)
        for (size_t c = 0; c < M; ++c) {
            const epik_amd_correlation& r = records[c * N + b];
            out += std::to_string(b) + '\t' + columns[c] + '\t' + g17_or_na(r.mass_pearson) + '\t' + g17_or_na(r.mass_spearman) + '\t' +
                   g17_or_na(r.imbalance_pearson) + '\t' + g17_or_na(r.imbalance_spearman) + '\n';
        }
    return out;
}

std::string format_dispersion_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals, uint32_t num_branches,
                                  const epik_amd_dispersion* records)
{
    std::string out = used_head(samples, totals, "dispersion", "");
    out += "edge_num\tmass_mean\tmass_var\tmass_sd\tmass_cv\tmass_vmr\timbalance_mean\timbalance_var\timbalance_sd\n";
    for (size_t b = 0; b < num_branches; ++b) {
        const epik_amd_dispersion& r = records[b];
        out += std::to_string(b);
        for (const double v : {r.mass_mean, r.mass_var, r.mass_sd, r.mass_cv, r.mass_vmr, r.imbalance_mean, r.imbalance_var, r.imbalance_sd})
            out += '\t' + g17_or_na(v);
        out += '\n';
    }
    return out;
}

std::string format_permanova_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                                 const std::vector<std::string>& columns, const std::vector<std::vector<std::string>>& names,
                                 const uint32_t* labels, uint32_t num_permutations, uint64_t seed, bool pairwise,
                                 const epik_amd_permanova* records, const double* group_ss, uint32_t distance)
{
    const size_t S = samples.size(), M = columns.size(), slots = 1 + (pairwise ? EPIK_AMD_PERMANOVA_PAIR_SLOTS : 0);
    std::string out = used_head(samples, totals, "permanova",
                                " columns=" + std::to_string(M) + " permutations=" + std::to_string(num_permutations) +
                                    " seed=" + std::to_string(seed) + " pairwise=" + (pairwise ? "1" : "0") + distance_field(distance));
    // the groups of every column in the rule's order: by first appearance among the used samples
    std::vector<std::vector<uint32_t>> label_of(M), size_of(M);
    for (size_t c = 0; c < M; ++c) {
        std::map<uint32_t, uint32_t> group_of;
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (totals[s] == 0 || v == EPIK_AMD_PERMANOVA_MISSING) continue;
            const auto [it, fresh] = group_of.emplace(v, (uint32_t)label_of[c].size());
            if (fresh) label_of[c].push_back(v), size_of[c].push_back(0);
            ++size_of[c][it->second];
        }
    }
    for (size_t c = 0; c < M; ++c)
        out += "# column\t" + std::to_string(c) + '\t' + columns[c] + '\t' + std::to_string(records[c * slots].used) + '\t' +
               std::to_string(records[c * slots].groups) + '\n';
    for (size_t c = 0; c < M; ++c)
        for (size_t g = 0; g < label_of[c].size(); ++g)
            out += "# group\t" + std::to_string(c) + '\t' + std::to_string(g) + '\t' + names[c][label_of[c][g]] + '\t' +
                   std::to_string(size_of[c][g]) + '\t' + g17_or_na(group_ss[c * EPIK_AMD_PERMANOVA_MAX_GROUPS + g]) + '\n';
    out += "column\ta\tb\tused\tgroups\tss_total\tss_among\tss_within\tf\tr2\tat_most\tp\n";
    const auto line = [&](size_t c, const std::string& a, const std::string& b, const epik_amd_permanova& r) {
        const double among = std::isnan(r.ss_total) ? r.ss_total : r.ss_total - r.ss_within;
        out += columns[c] + '\t' + a + '\t' + b + '\t' + std::to_string(r.used) + '\t' + std::to_string(r.groups) + '\t' +
               g17_or_na(r.ss_total) + '\t' + g17_or_na(among) + '\t' + g17_or_na(r.ss_within) + '\t' + g17_or_na(r.f) + '\t' +
               g17_or_na(r.r2) + '\t' + std::to_string(r.at_most) + '\t' + g17_or_na(r.p) + '\n';
    };
    for (size_t c = 0; c < M; ++c) {
        line(c, "*", "*", records[c * slots]);
        if (!pairwise) continue;
        for (size_t h = 1; h < label_of[c].size(); ++h)
            for (size_t g = 0; g < h; ++g)
                line(c, names[c][label_of[c][g]], names[c][label_of[c][h]], records[c * slots + 1 + h * (h - 1) / 2 + g]);
    }
    return out;
}

std::string format_edgetest_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                                const std::vector<std::string>& columns, const std::vector<std::vector<std::string>>& names,
                                const uint32_t* labels, uint32_t num_branches, uint32_t num_permutations, uint64_t seed,
                                const epik_amd_edgetest* records)
{
    const size_t S = samples.size(), M = columns.size(), N = num_branches;
    std::string out = used_head(samples, totals, "edgetest",
                                " columns=" + std::to_string(M) + " permutations=" + std::to_string(num_permutations) +
                                    " seed=" + std::to_string(seed));
    // the groups of every column in the rule's order: by first appearance among the used samples
    std::vector<std::vector<uint32_t>> label_of(M), size_of(M);
    for (size_t c = 0; c < M; ++c) {
        std::map<uint32_t, uint32_t> group_of;
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (totals[s] == 0 || v == EPIK_AMD_EDGETEST_MISSING) continue;
            const auto [it, fresh] = group_of.emplace(v, (uint32_t)label_of[c].size());
            if (fresh) label_of[c].push_back(v), size_of[c].push_back(0);
            ++size_of[c][it->second];
        }
    }
    for (size_t c = 0; c < M; ++c)
        out += "# column\t" + std::to_string(c) + '\t' + columns[c] + '\t' + std::to_string(records[c * N].used) + '\t' +
               std::to_string(records[c * N].groups) + '\n';
    for (size_t c = 0; c < M; ++c)
        for (size_t g = 0; g < label_of[c].size(); ++g)
            out += "# group\t" + std::to_string(c) + '\t' + std::to_string(g) + '\t' + names[c][label_of[c][g]] + '\t' +
                   std::to_string(size_of[c][g]) + '\n';
    out += "edge_num\tcolumn";
    for (const char* kind : {"mass", "imbalance"})
        for (const char* field : {"eta2", "f", "p", "p_adj", "top", "h", "kw_p", "kw_p_adj"}) out += std::string("\t") + kind + '_' + field;
    out += '\n';
    for (size_t c = 0; c < M; ++c)
        for (size_t b = 0; b < N; ++b) {
            const epik_amd_edgetest& r = records[c * N + b];
            bool any = false;
            for (const auto& fam : r.family) any = any || !std::isnan(fam.eta2);
            if (!any) continue;
            out += std::to_string(b) + '\t' + columns[c];
            for (size_t kind = 0; kind < 2; ++kind) {
                const epik_amd_edgetest_family &plain = r.family[2 * kind], &ranks = r.family[2 * kind + 1];
                const uint32_t top = kind ? r.top_imbalance : r.top_mass;
                out += '\t' + g17_or_na(plain.eta2) + '\t' + g17_or_na(plain.stat) + '\t' + g17_or_na(plain.p) + '\t' +
                       g17_or_na(plain.p_adj) + '\t' + (top == EPIK_AMD_EDGETEST_MISSING ? std::string("NA") : names[c][label_of[c][top]]) +
                       '\t' + g17_or_na(ranks.stat) + '\t' + g17_or_na(ranks.p) + '\t' + g17_or_na(ranks.p_adj);
            }
            out += '\n';
        }
    return out;
}

std::string format_permdisp_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                                const std::vector<std::string>& columns, const std::vector<std::vector<std::string>>& names,
                                const uint32_t* labels, uint32_t num_permutations, uint64_t seed, bool pairwise,
                                const epik_amd_permdisp* records, const double* group_mean, const double* z, uint32_t distance)
{
    const size_t S = samples.size(), M = columns.size(), slots = 1 + (pairwise ? EPIK_AMD_PERMDISP_PAIR_SLOTS : 0);
    std::string out = used_head(samples, totals, "permdisp",
                                " columns=" + std::to_string(M) + " permutations=" + std::to_string(num_permutations) +
                                    " seed=" + std::to_string(seed) + " pairwise=" + (pairwise ? "1" : "0") + distance_field(distance));
    // the groups of every column in the rule's order: by first appearance among the used samples
    std::vector<std::vector<uint32_t>> label_of(M), size_of(M);
    for (size_t c = 0; c < M; ++c) {
        std::map<uint32_t, uint32_t> group_of;
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (totals[s] == 0 || v == EPIK_AMD_PERMDISP_MISSING) continue;
            const auto [it, fresh] = group_of.emplace(v, (uint32_t)label_of[c].size());
            if (fresh) label_of[c].push_back(v), size_of[c].push_back(0);
            ++size_of[c][it->second];
        }
    }
    for (size_t c = 0; c < M; ++c)
        out += "# column\t" + std::to_string(c) + '\t' + columns[c] + '\t' + std::to_string(records[c * slots].used) + '\t' +
               std::to_string(records[c * slots].groups) + '\n';
    for (size_t c = 0; c < M; ++c)
        for (size_t g = 0; g < label_of[c].size(); ++g)
            out += "# group\t" + std::to_string(c) + '\t' + std::to_string(g) + '\t' + names[c][label_of[c][g]] + '\t' +
                   std::to_string(size_of[c][g]) + '\t' + g17_or_na(group_mean[c * EPIK_AMD_PERMDISP_MAX_GROUPS + g]) + '\n';
    out += "column\ta\tb\tused\tgroups\tclipped\teta2\tf\tat_least\tp\n";
    const auto line = [&](size_t c, const std::string& a, const std::string& b, const epik_amd_permdisp& r) {
        out += columns[c] + '\t' + a + '\t' + b + '\t' + std::to_string(r.used) + '\t' + std::to_string(r.groups) + '\t' +
               std::to_string(r.clipped) + '\t' + g17_or_na(r.eta2) + '\t' + g17_or_na(r.f) + '\t' + std::to_string(r.at_least) + '\t' +
               g17_or_na(r.p) + '\n';
    };
    for (size_t c = 0; c < M; ++c) {
        line(c, "*", "*", records[c * slots]);
        if (!pairwise) continue;
        for (size_t h = 1; h < label_of[c].size(); ++h)
            for (size_t g = 0; g < h; ++g)
                line(c, names[c][label_of[c][g]], names[c][label_of[c][h]], records[c * slots + 1 + h * (h - 1) / 2 + g]);
    }
    out += "# distances\ncolumn\tname\tlabel\tdistance\n";
    for (size_t c = 0; c < M; ++c)
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (totals[s] == 0 || v == EPIK_AMD_PERMDISP_MISSING) continue;
            out += columns[c] + '\t' + samples[s].name + '\t' + names[c][v] + '\t' + g17_or_na(z[c * S + s]) + '\n';
        }
    return out;
}

namespace {

// the lines of a design that cohort_model and cohort_edgemodel .tsv share: "# unused", "# incomplete", "# term", "# group" and
// "# aliased", from the columns and the accepted columns of every term and the aliased bytes
std::string design_lines(const std::vector<cohort_sample>& samples, const uint64_t* totals, const cohort_design& design,
                         const std::vector<uint32_t>& columns_of, const std::vector<uint32_t>& df_of, const uint8_t* aliased)
{
    const size_t S = samples.size(), T = design.terms.size();
    std::string out;
    for (size_t s = 0; s < S; ++s)
        if (totals[s] == 0) out += "# unused\t" + samples[s].name + "\n";
    const auto lacks = [&](size_t s, size_t t) {
        return design.kind[t] ? std::isnan(design.values[s * T + t]) : design.labels[s * T + t] == EPIK_AMD_MODEL_MISSING;
    };
    std::vector<size_t> used;
    for (size_t s = 0; s < S; ++s) {
        if (totals[s] == 0) continue;
        size_t t = 0;
        while (t < T && !lacks(s, t)) ++t;
        if (t == T)
            used.push_back(s);
        else
            out += "# incomplete\t" + samples[s].name + "\t" + design.terms[t] + "\n";
    }
    for (size_t t = 0; t < T; ++t)
        out += "# term\t" + std::to_string(t) + (design.kind[t] ? "\tn\t" : "\tf\t") + design.terms[t] + "\t" +
               std::to_string(columns_of[t]) + "\t" + std::to_string(df_of[t]) + "\n";
    // the groups of the factor terms in the rule's order, and the label of every column
    std::vector<std::string> column_label;
    std::vector<size_t> column_term;
    std::string groups;
    for (size_t t = 0; t < T; ++t) {
        if (design.kind[t]) {
            column_label.push_back("-"), column_term.push_back(t);
            continue;
        }
        std::vector<uint32_t> order, size_of(EPIK_AMD_MODEL_MAX_GROUPS, 0);
        for (const size_t s : used) {
            const uint32_t v = design.labels[s * T + t];
            if (v >= EPIK_AMD_MODEL_MAX_GROUPS) continue;
            if (!size_of[v]) order.push_back(v);
            ++size_of[v];
        }
        for (size_t g = 0; g < order.size(); ++g) {
            groups += "# group\t" + std::to_string(t) + "\t" + std::to_string(g) + "\t" + design.names[t][order[g]] + "\t" +
                      std::to_string(size_of[order[g]]) + "\n";
            if (g) column_label.push_back(design.names[t][order[g]]), column_term.push_back(t);
        }
    }
    out += groups;
    for (size_t c = 0; c < column_label.size() && c < EPIK_AMD_MODEL_MAX_COLUMNS; ++c)
        if (aliased[c]) out += "# aliased\t" + std::to_string(column_term[c]) + "\t" + column_label[c] + "\n";
    return out;
}

}  // namespace

std::string format_model_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals, const cohort_design& design,
                             uint32_t num_permutations, uint64_t seed, const epik_amd_model_term* records,
                             const epik_amd_model_info& info, const uint8_t* aliased, uint32_t distance)
{
    const size_t S = samples.size(), T = design.terms.size();
    std::string out = "# epik_amd model v1  samples=" + std::to_string(S) + " used=" + std::to_string(info.used) +
                      " terms=" + std::to_string(T) + " columns=" + std::to_string(info.columns) + " rank=" + std::to_string(info.rank) +
                      " permutations=" + std::to_string(num_permutations) + " seed=" + std::to_string(seed) + distance_field(distance) + "\n";
    std::vector<uint32_t> columns_of(T), df_of(T);
    for (size_t t = 0; t < T; ++t) columns_of[t] = records[t].columns, df_of[t] = records[t].df;
    out += design_lines(samples, totals, design, columns_of, df_of, aliased);
    out += "term\tdf\tss\tr2\tf\tat_least\tp\n";
    double rest = 1.0;
    for (size_t k = 0; k <= T; ++k) {
        const epik_amd_model_term& r = records[k];
        out += (k < T ? design.terms[k] : std::string("model")) + "\t" + std::to_string(r.df) + "\t" + g17_or_na(r.ss) + "\t" +
               g17_or_na(r.r2) + "\t" + g17_or_na(r.f) + "\t" + (std::isnan(r.p) ? std::string("NA") : std::to_string(r.at_least)) + "\t" +
               g17_or_na(r.p) + "\n";
        if (k < T && r.df && !std::isnan(r.r2)) rest = rest - r.r2;
    }
    const bool total = info.ss_total > 0.0;
    out += "residual\t" + std::to_string(info.df_res) + "\t" + g17(info.ss_res) + "\t" + (total ? g17(rest) : std::string("NA")) +
           "\tNA\tNA\tNA\n";
    out += "total\t" + std::to_string((int64_t)info.used - 1) + "\t" + g17(info.ss_total) + "\t" + (total ? "1" : "NA") + "\tNA\tNA\tNA\n";
    return out;
}

std::string format_edgemodel_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals, const cohort_design& design,
                                 uint32_t num_branches, uint32_t num_permutations, uint64_t seed, const epik_amd_edgemodel* records,
                                 const epik_amd_edgemodel_info& info, const uint8_t* aliased)
{
    const size_t S = samples.size(), T = design.terms.size(), N = num_branches;
    std::string out = "# epik_amd edgemodel v1  samples=" + std::to_string(S) + " used=" + std::to_string(info.used) +
                      " terms=" + std::to_string(T) + " columns=" + std::to_string(info.columns) + " rank=" + std::to_string(info.rank) +
                      " permutations=" + std::to_string(num_permutations) + " seed=" + std::to_string(seed) + "\n";
    out += design_lines(samples, totals, design, std::vector<uint32_t>(info.term_columns, info.term_columns + T),
                        std::vector<uint32_t>(info.df, info.df + T), aliased);
    out += "term\tedge_num";
    for (const char* kind : {"mass", "imbalance"})
        for (const char* field : {"ss", "r2", "partial_r2", "f", "sign", "p", "p_adj"}) out += std::string("\t") + kind + '_' + field;
    out += '\n';
    for (size_t t = 0; t < T; ++t)
        for (size_t b = 0; b < N; ++b) {
            const epik_amd_edgemodel& r = records[t * N + b];
            if (std::isnan(r.family[0].ss) && std::isnan(r.family[1].ss)) continue;
            out += design.terms[t] + '\t' + std::to_string(b);
            for (const auto& fam : r.family)
                out += '\t' + g17_or_na(fam.ss) + '\t' + g17_or_na(fam.r2) + '\t' + g17_or_na(fam.partial_r2) + '\t' + g17_or_na(fam.f) +
                       '\t' + (std::isnan(fam.ss) ? std::string("NA") : std::to_string(fam.sign)) + '\t' + g17_or_na(fam.p) + '\t' +
                       g17_or_na(fam.p_adj);
            out += '\n';
        }
    return out;
}

cohort_matrix read_cohort_matrix(const std::string& file, const std::vector<cohort_sample>& samples, const char* flag)
{
    std::ifstream in(file);
    if (!in) throw std::runtime_error(std::string(flag) + ": cannot open " + file);
    const size_t S = samples.size();
    std::map<std::string, size_t> index_of;
    for (size_t s = 0; s < S; ++s) index_of[samples[s].name] = s;
    cohort_matrix out;
    out.matrix.assign(S * S, 0.0), out.present.assign(S, 0);
    const auto fail = [&](size_t line_no, const std::string& what) {
        throw std::runtime_error(std::string(flag) + ": " + file + ", line " + std::to_string(line_no) + ": " + what);
    };
    std::vector<std::string> header;        // the names of the first line
    std::vector<size_t> target;             // their samples, or S for a name outside the list
    std::map<std::string, size_t> column_of;
    std::vector<size_t> row_line;           // the line of every name's row, 0: none yet
    std::vector<std::vector<double>> rows;  // by the first line's order
    size_t line_no = 0;
    for (std::string line; std::getline(in, line);) {
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::vector<std::string> fields = split_tabs(line);
        if (header.empty()) {
            if (fields.size() < 2 || fields[0] != "name") fail(line_no, "the first line must be name<TAB>name1<TAB>...");
            for (size_t c = 1; c < fields.size(); ++c) {
                if (fields[c].empty()) fail(line_no, "column " + std::to_string(c) + ": an empty name");
                if (!column_of.emplace(fields[c], c - 1).second)
                    fail(line_no, "column " + std::to_string(c) + ": the name '" + fields[c] + "' is given twice");
                header.push_back(fields[c]);
                const auto it = index_of.find(fields[c]);
                target.push_back(it == index_of.end() ? S : it->second);
            }
            row_line.assign(header.size(), 0), rows.assign(header.size(), {});
            continue;
        }
        if (fields.size() != header.size() + 1)
            fail(line_no, std::to_string(fields.size()) + " fields, the first line has " + std::to_string(header.size() + 1));
        const auto it = column_of.find(fields[0]);
        if (it == column_of.end()) fail(line_no, "the name '" + fields[0] + "' is not in the first line");
        const size_t r = it->second;
        if (row_line[r]) fail(line_no, "the name '" + fields[0] + "' is given twice (line " + std::to_string(row_line[r]) + ")");
        row_line[r] = line_no;
        rows[r].resize(header.size());
        for (size_t c = 0; c < header.size(); ++c) {
            const std::string& cell = fields[c + 1];
            const std::string where = "column " + std::to_string(c + 1) + " (" + header[c] + "): ";
            if (!is_number(cell)) fail(line_no, where + "'" + cell + "' is not a number");
            const double v = std::strtod(cell.c_str(), nullptr);
            if (c != r && (!(v >= 0.0) || !std::isfinite(v))) fail(line_no, where + "the distance " + cell + " is negative or not finite");
            rows[r][c] = v;
            if (c != r && row_line[c] && rows[c][r] != v)
                fail(line_no, where + "the distance " + cell + " differs from its mirror cell (line " + std::to_string(row_line[c]) + ")");
        }
    }
    if (header.empty()) throw std::runtime_error(std::string(flag) + ": " + file + " has no first line of names");
    for (size_t r = 0; r < header.size(); ++r)
        if (!row_line[r]) throw std::runtime_error(std::string(flag) + ": " + file + " has no row for the name '" + header[r] + "'");
    for (size_t r = 0; r < header.size(); ++r) {
        if (target[r] == S) {
            ++out.skipped;
            continue;
        }
        out.present[target[r]] = 1;
        for (size_t c = 0; c < header.size(); ++c)
            if (target[c] != S && c != r) out.matrix[target[r] * S + target[c]] = rows[r][c];
    }
    return out;
}

cohort_mantel_sides read_cohort_mantel_sides(const std::string& metadata_file, const std::vector<std::string>& matrix_arguments,
                                             const std::string& partial, const std::vector<cohort_sample>& samples)
{
    const size_t S = samples.size();
    cohort_mantel_sides out;
    if (!metadata_file.empty()) {
        const cohort_metadata meta = read_cohort_metadata(metadata_file, samples);
        const size_t M = meta.columns.size();
        out.names = meta.columns, out.num_columns = (uint32_t)M, out.skipped = meta.skipped;
        out.values.resize(M * S);
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < M; ++c) out.values[c * S + s] = meta.values[s * M + c];
    }
    if (matrix_arguments.size() > EPIK_AMD_MANTEL_MAX_MATRICES)
        throw std::runtime_error("--cohort-mantel-matrix is given " + std::to_string(matrix_arguments.size()) + " times, 8 at the most");
    for (const std::string& argument : matrix_arguments) {
        const size_t eq = argument.find('=');
        if (eq == std::string::npos || eq == 0 || eq + 1 == argument.size())
            throw std::runtime_error("--cohort-mantel-matrix " + argument + ": the argument must be NAME=FILE");
        const std::string name = argument.substr(0, eq);
        if (std::find(out.names.begin(), out.names.end(), name) != out.names.end())
            throw std::runtime_error("--cohort-mantel-matrix " + argument + ": the name '" + name + "' is given twice");
        const cohort_matrix m = read_cohort_matrix(argument.substr(eq + 1), samples);
        out.names.push_back(name), ++out.num_matrices, out.skipped += m.skipped;
        out.matrices.insert(out.matrices.end(), m.matrix.begin(), m.matrix.end());
        out.present.insert(out.present.end(), m.present.begin(), m.present.end());
    }
    if (out.names.empty()) throw std::runtime_error("the Mantel test needs --cohort-mantel or --cohort-mantel-matrix (a side)");
    if (!partial.empty()) {
        const auto it = std::find(out.names.begin(), out.names.end(), partial);
        if (it == out.names.end())
            throw std::runtime_error("--cohort-mantel-partial: '" + partial + "' names no column of --cohort-mantel and no matrix");
        out.control = (uint32_t)(it - out.names.begin());
    }
    return out;
}

const char* mantel_method_name(uint32_t methods)
{
    return methods == EPIK_AMD_MANTEL_PEARSON ? "pearson" : methods == EPIK_AMD_MANTEL_SPEARMAN ? "spearman" : "both";
}

uint32_t mantel_methods_of_name(const std::string& name)
{
    return name == "pearson" ? EPIK_AMD_MANTEL_PEARSON
           : name == "spearman" ? EPIK_AMD_MANTEL_SPEARMAN
           : name == "both"     ? (EPIK_AMD_MANTEL_PEARSON | EPIK_AMD_MANTEL_SPEARMAN)
                                : 0u;
}

std::string format_mantel_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                              const std::vector<std::string>& side_names, uint32_t num_columns, uint32_t methods, uint32_t control,
                              uint32_t num_permutations, uint64_t seed, const epik_amd_mantel* records, uint32_t distance)
{
    const size_t Q = side_names.size(), per_side = (methods & 1u) + (methods >> 1 & 1u);
    std::string out = used_head(samples, totals, "mantel",
                                " sides=" + std::to_string(Q) + " permutations=" + std::to_string(num_permutations) +
                                    " seed=" + std::to_string(seed) + " method=" + mantel_method_name(methods) + " partial=" +
                                    (control == EPIK_AMD_MANTEL_NO_CONTROL ? std::string("-") : side_names[control]) +
                                    distance_field(distance));
    for (size_t q = 0; q < Q; ++q)
        out += "# side\t" + std::to_string(q) + '\t' + (q < num_columns ? "column" : "matrix") + '\t' + side_names[q] + '\t' +
               std::to_string(records[q * per_side].used) + '\n';
    out += "side\tmethod\tused\tr\tr_xz\tr_yz\tstat\tat_least\tp\n";
    for (size_t e = 0; e < Q * per_side; ++e) {
        const epik_amd_mantel& r = records[e];
        out += side_names[r.side] + '\t' + (r.method ? "spearman" : "pearson") + '\t' + std::to_string(r.used) + '\t' + g17_or_na(r.r) +
               '\t' + g17_or_na(r.r_xz) + '\t' + g17_or_na(r.r_yz) + '\t' + g17_or_na(r.stat) + '\t' + std::to_string(r.at_least) + '\t' +
               g17_or_na(r.p) + '\n';
    }
    return out;
}

std::string format_anosim_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                              const std::vector<std::string>& columns, const std::vector<std::vector<std::string>>& names,
                              const uint32_t* labels, uint32_t num_permutations, uint64_t seed, const epik_amd_anosim* records,
                              uint32_t distance)
{
    const size_t S = samples.size(), M = columns.size();
    std::string out = used_head(samples, totals, "anosim",
                                " columns=" + std::to_string(M) + " permutations=" + std::to_string(num_permutations) +
                                    " seed=" + std::to_string(seed) + distance_field(distance));
    for (size_t c = 0; c < M; ++c)
        out += "# column\t" + std::to_string(c) + '\t' + columns[c] + '\t' + std::to_string(records[c].used) + '\t' +
               std::to_string(records[c].groups) + '\n';
    for (size_t c = 0; c < M; ++c) {  // the groups in the rule's order: by first appearance among the used samples
        std::map<uint32_t, uint32_t> group_of;
        std::vector<uint32_t> label_of, size_of;
        for (size_t s = 0; s < S; ++s) {
            const uint32_t v = labels[s * M + c];
            if (totals[s] == 0 || v == EPIK_AMD_PERMANOVA_MISSING) continue;
            const auto [it, fresh] = group_of.emplace(v, (uint32_t)label_of.size());
            if (fresh) label_of.push_back(v), size_of.push_back(0);
            ++size_of[it->second];
        }
        for (size_t g = 0; g < label_of.size(); ++g)
            out += "# group\t" + std::to_string(c) + '\t' + std::to_string(g) + '\t' + names[c][label_of[g]] + '\t' +
                   std::to_string(size_of[g]) + '\n';
    }
    out += "column\tused\tgroups\tmean_between\tmean_within\tr\tat_least\tp\n";
    for (size_t c = 0; c < M; ++c) {
        const epik_amd_anosim& r = records[c];
        out += columns[c] + '\t' + std::to_string(r.used) + '\t' + std::to_string(r.groups) + '\t' + g17_or_na(r.mean_between) + '\t' +
               g17_or_na(r.mean_within) + '\t' + g17_or_na(r.r) + '\t' + std::to_string(r.at_least) + '\t' + g17_or_na(r.p) + '\n';
    }
    return out;
}

std::vector<uint32_t> read_cohort_strata(const std::string& file, const std::string& column, const std::vector<cohort_sample>& samples,
                                         std::string* name)
{
    const char* flag = "--cohort-strata";
    const cohort_factors factors = read_cohort_factors(file, samples, false, (size_t)-1, flag);  // (no cap: a pair a label)
    const size_t M = factors.columns.size();
    size_t c = 0;
    if (column.empty()) {
        if (M != 1)
            throw std::runtime_error(std::string(flag) + ": " + file + " has " + std::to_string(M) +
                                     " columns: --cohort-strata-column must name one");
    } else {
        c = (size_t)(std::find(factors.columns.begin(), factors.columns.end(), column) - factors.columns.begin());
        if (c == M) throw std::runtime_error("--cohort-strata-column: " + file + " has no column '" + column + "'");
    }
    std::vector<uint32_t> strata(samples.size());
    for (size_t s = 0; s < samples.size(); ++s) {
        strata[s] = factors.labels[s * M + c];
        if (strata[s] != EPIK_AMD_PERMANOVA_MISSING) continue;
        std::ifstream in(file);  // the sample's line, for the message: the reader has seen it
        std::string line;
        size_t number = 1;
        for (; std::getline(in, line); ++number)
            if (!line.empty() && line[0] != '#' && split_tabs(line)[0] == samples[s].name) break;
        throw std::runtime_error(std::string(flag) + ": " + file + " line " + std::to_string(number) + ", column " + factors.columns[c] +
                                 ": the sample '" + samples[s].name + "' has no stratum");
    }
    if (name) *name = factors.columns[c];
    return strata;
}

std::string with_strata_field(std::string text, const std::string& name)
{
    if (!name.empty()) text.insert(std::min(text.find('\n'), text.size()), "\tstrata=" + name);
    return text;
}

bool constant_within_strata(const uint32_t* labels, size_t S, size_t M, size_t c, uint32_t missing, const uint64_t* totals,
                            const uint32_t* strata)
{
    std::map<uint32_t, uint32_t> label_of;
    for (size_t s = 0; s < S; ++s) {
        const uint32_t v = labels[s * M + c];
        if (totals[s] == 0 || v == missing) continue;
        if (!label_of.emplace(strata[s], v).second && label_of[strata[s]] != v) return false;
    }
    return true;
}

void write_through_part(const std::string& filename, const std::string& text)
{
    const std::string part = filename + ".part";
    {
        std::ofstream out(part, std::ios::binary);
        out << text;
        out.close();
        if (!out) throw std::runtime_error("Could not write " + part);
    }
    if (std::rename(part.c_str(), filename.c_str()) != 0) throw std::runtime_error("Could not write " + filename);
}

}  // namespace epik_amd
