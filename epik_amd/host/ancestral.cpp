// ancestral.cpp -- the host mirror of the ancestral reconstruction (ancestral.hpp): per site a down pass, an up pass and
// the ghost nodes of every branch, sites handed out to threads; and the model side: P(t) by a Jacobi
// eigendecomposition of the symmetrised rate matrix, discrete-gamma rates from an incomplete gamma function written here.
#include "ancestral.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "parallel.hpp"

namespace epik_amd {

namespace {

int invalid(std::string &err, const std::string &what)
{
    err = what;
    return EPIK_AMD_ERR_INVALID;
}

// the states of a mask as 1.0 / 0.0; none of the sigma low bits: all
inline void mask_vector(uint32_t mask, uint32_t S, double *out)
{
    const uint32_t full = S == 32 ? 0xffffffffu : (1u << S) - 1;
    uint32_t m = mask & full;
    if (m == 0) m = full;
    for (uint32_t y = 0; y < S; ++y) out[y] = (m >> y & 1u) ? 1.0 : 0.0;
}

// out[x] = sum over y of P[x][y] * v[y], from the first term
inline void apply(const double *P, const double *v, uint32_t S, double *out)
{
    for (uint32_t x = 0; x < S; ++x) {
        const double *row = P + (size_t)x * S;
        double acc = row[0] * v[0];
        for (uint32_t y = 1; y < S; ++y) acc = acc + row[y] * v[y];
        out[x] = acc;
    }
}

// the site's C * S entries brought to a maximum in [0.5, 1)
inline void rescale(double *e, uint32_t n)
{
    double m = 0.0;
    for (uint32_t i = 0; i < n; ++i)
        if (e[i] > m) m = e[i];
    if (!(m > 0.0)) return;
    int ex = 0;
    (void)std::frexp(m, &ex);
    for (uint32_t i = 0; i < n; ++i) e[i] = std::ldexp(e[i], -ex);
}

struct SiteWork {
    std::vector<double> D, U, leaf, fa, fb, t, num, numb;
};

// n[x] / Z rounded to float32, or a row of zeros
inline bool write_row(const double *num, uint32_t S, float *out)
{
    double Z = num[0];
    for (uint32_t x = 1; x < S; ++x) Z = Z + num[x];
    if (!(Z > 0.0) || !std::isfinite(Z)) {
        for (uint32_t x = 0; x < S; ++x) out[x] = 0.0f;
        return false;
    }
    for (uint32_t x = 0; x < S; ++x) out[x] = (float)(num[x] / Z);
    return true;
}

uint64_t one_site(const epik_amd_ancestral_desc &d, const ancestral_tree &tree, const uint32_t *masks, uint64_t L, uint64_t s,
                  uint32_t ghosts, float *post, SiteWork &w)
{
    const uint32_t N = d.num_nodes, S = d.sigma, C = d.num_categories, CS = C * S;
    const size_t mat = (size_t)S * S;
    w.D.resize((size_t)tree.n_inner * CS), w.U.resize((size_t)N * CS), w.leaf.resize(2 * (size_t)S);
    w.fa.resize(S), w.fb.resize(S), w.t.resize(S), w.num.resize(S), w.numb.resize(S);
    // D of node u in category c: its vector of S values (a leaf's is the same in every category)
    const auto down_of = [&](uint32_t u, uint32_t c, double *leaf) -> const double * {
        if (tree.left[u] == kAncestralNone) {
            mask_vector(masks[(uint64_t)tree.leaf_row[u] * L + s], S, leaf);
            return leaf;
        }
        return w.D.data() + (size_t)tree.inner_slot[u] * CS + (size_t)c * S;
    };
    for (const auto &level : tree.down_levels)
        for (const uint32_t v : level) {
            const uint32_t l = tree.left[v], r = tree.right[v];
            double *out = w.D.data() + (size_t)tree.inner_slot[v] * CS;
            for (uint32_t c = 0; c < C; ++c) {
                apply(d.p_full + ((size_t)l * C + c) * mat, down_of(l, c, w.leaf.data()), S, w.fa.data());
                apply(d.p_full + ((size_t)r * C + c) * mat, down_of(r, c, w.leaf.data() + S), S, w.fb.data());
                for (uint32_t x = 0; x < S; ++x) out[(size_t)c * S + x] = w.fa[x] * w.fb[x];
            }
            rescale(out, CS);
        }
    for (const auto &level : tree.up_levels)
        for (const uint32_t v : level) {
            const uint32_t p = (uint32_t)d.parent[v], sib = tree.sibling[v];
            double *out = w.U.data() + (size_t)v * CS;
            for (uint32_t c = 0; c < C; ++c) {
                apply(d.p_full + ((size_t)sib * C + c) * mat, down_of(sib, c, w.leaf.data()), S, w.fa.data());
                if (p == N - 1) {
                    for (uint32_t x = 0; x < S; ++x) out[(size_t)c * S + x] = w.fa[x];
                } else {
                    apply(d.p_full + ((size_t)p * C + c) * mat, w.U.data() + (size_t)p * CS + (size_t)c * S, S, w.fb.data());
                    for (uint32_t x = 0; x < S; ++x) out[(size_t)c * S + x] = w.fa[x] * w.fb[x];
                }
            }
            rescale(out, CS);
        }
    uint64_t dead = 0;
    const bool inner = ghosts != EPIK_AMD_GHOSTS_OUTER, outer = ghosts != EPIK_AMD_GHOSTS_INNER;
    const uint64_t outer_base = ghosts == EPIK_AMD_GHOSTS_BOTH ? N - 1 : 0;
    for (uint32_t b = 0; b + 1 < N; ++b) {
        for (uint32_t c = 0; c < C; ++c) {
            const double *h = d.p_half + ((size_t)b * C + c) * mat;
            apply(h, down_of(b, c, w.leaf.data()), S, w.fa.data());
            apply(h, w.U.data() + (size_t)b * CS + (size_t)c * S, S, w.fb.data());
            for (uint32_t x = 0; x < S; ++x) w.t[x] = d.pi[x] * (w.fa[x] * w.fb[x]);
            for (uint32_t x = 0; x < S; ++x) w.num[x] = c == 0 ? d.weights[0] * w.t[x] : w.num[x] + d.weights[c] * w.t[x];
            if (outer) {
                const double *q = d.p_pend + ((size_t)b * C + c) * mat;
                for (uint32_t y = 0; y < S; ++y) {
                    double acc = w.t[0] * q[y];
                    for (uint32_t x = 1; x < S; ++x) acc = acc + w.t[x] * q[(size_t)x * S + y];
                    w.numb[y] = c == 0 ? d.weights[0] * acc : w.numb[y] + d.weights[c] * acc;
                }
            }
        }
        if (inner && !write_row(w.num.data(), S, post + ((uint64_t)b * L + s) * S)) ++dead;
        if (outer && !write_row(w.numb.data(), S, post + ((outer_base + b) * L + s) * S)) ++dead;
    }
    return dead;
}

}  // namespace

int ancestral_check(const epik_amd_ancestral_desc &d, ancestral_tree &tree, std::string &err)
{
    const uint32_t N = d.num_nodes, S = d.sigma, C = d.num_categories;
    if (S != 4 && S != 20) return invalid(err, "sigma = " + std::to_string(S) + " is neither 4 nor 20");
    if (C < 1 || C > kAncestralMaxCategories)
        return invalid(err, "num_categories = " + std::to_string(C) + " is outside [1, " + std::to_string(kAncestralMaxCategories) + "]");
    if (N < 3 || N > 0x7fffffffu) return invalid(err, "a rooted binary tree has at least 3 nodes (num_nodes is " + std::to_string(N) + ")");
    if (!d.parent || !d.weights || !d.pi || !d.p_full || !d.p_half || !d.p_pend) return invalid(err, "null array in the descriptor");
    tree = ancestral_tree{};
    tree.N = N;
    tree.left.assign(N, kAncestralNone), tree.right.assign(N, kAncestralNone), tree.sibling.assign(N, kAncestralNone);
    tree.leaf_row.assign(N, kAncestralNone), tree.inner_slot.assign(N, kAncestralNone);
    if (d.parent[N - 1] != -1) return invalid(err, "parent[" + std::to_string(N - 1) + "] must be -1: the root is the last node");
    for (uint32_t v = 0; v + 1 < N; ++v) {
        const int64_t p = d.parent[v];
        if (p <= (int64_t)v || p >= (int64_t)N)
            return invalid(err, "parent[" + std::to_string(v) + "] = " + std::to_string(p) + " is not a later node: the numbering must be post-order");
        if (tree.left[p] == kAncestralNone)
            tree.left[p] = v;
        else if (tree.right[p] == kAncestralNone)
            tree.right[p] = v;
        else
            return invalid(err, "node " + std::to_string(p) + " has more than two children: the tree must be binary");
    }
    std::vector<uint32_t> height(N, 0), depth(N, 0);
    for (uint32_t v = 0; v < N; ++v) {
        if (tree.left[v] == kAncestralNone) {
            tree.leaf_row[v] = tree.n_leaves++;
            continue;
        }
        if (tree.right[v] == kAncestralNone) return invalid(err, "node " + std::to_string(v) + " has one child: the tree must be binary");
        tree.inner_slot[v] = tree.n_inner++;
        tree.sibling[tree.left[v]] = tree.right[v], tree.sibling[tree.right[v]] = tree.left[v];
        height[v] = 1 + std::max(height[tree.left[v]], height[tree.right[v]]);
    }
    tree.down_levels.assign(height[N - 1], {});
    for (uint32_t v = 0; v < N; ++v)
        if (height[v]) tree.down_levels[height[v] - 1].push_back(v);
    uint32_t deepest = 0;
    for (uint32_t v = N - 1; v-- > 0;) depth[v] = depth[d.parent[v]] + 1, deepest = std::max(deepest, depth[v]);
    tree.up_levels.assign(deepest, {});
    for (uint32_t v = 0; v + 1 < N; ++v) tree.up_levels[depth[v] - 1].push_back(v);
    for (uint32_t c = 0; c < C; ++c)
        if (!(d.weights[c] >= 0.0) || !std::isfinite(d.weights[c]))
            return invalid(err, "weights[" + std::to_string(c) + "] is not a finite number that is at least 0");
    for (uint32_t x = 0; x < S; ++x)
        if (!(d.pi[x] >= 0.0) || !std::isfinite(d.pi[x])) return invalid(err, "pi[" + std::to_string(x) + "] is not a finite number that is at least 0");
    const uint64_t n = (uint64_t)(N - 1) * C * S * S;
    const double *tables[3] = {d.p_full, d.p_half, d.p_pend};
    const char *names[3] = {"p_full", "p_half", "p_pend"};
    for (int t = 0; t < 3; ++t)
        for (uint64_t i = 0; i < n; ++i)
            if (!(tables[t][i] >= 0.0 && tables[t][i] <= 2.0)) {
                const uint64_t y = i % S, x = i / S % S, c = i / S / S % C, b = i / S / S / C;
                return invalid(err, std::string(names[t]) + "[" + std::to_string(b) + "][" + std::to_string(c) + "][" + std::to_string(x) + "][" +
                                        std::to_string(y) + "] lies outside [0, 2]");
            }
    return EPIK_AMD_OK;
}

int ancestral_check_call(const void *masks, uint64_t L, uint32_t ghosts, std::string &err)
{
    if (ghosts > EPIK_AMD_GHOSTS_BOTH) return invalid(err, "ghosts = " + std::to_string(ghosts) + " is none of inner (0), outer (1), both (2)");
    if (L > 0xffffffffull) return invalid(err, "L = " + std::to_string(L) + " is 2^32 sites or more");
    if (L && !masks) return invalid(err, "null host buffer");
    return EPIK_AMD_OK;
}

void ancestral_branch_of(uint32_t N, uint32_t ghosts, uint32_t *branch_of)
{
    const uint64_t G = ancestral_ghost_count(N, ghosts);
    for (uint64_t g = 0; g < G; ++g) branch_of[g] = (uint32_t)(g % (N - 1));
}

void ancestral_rule_host(const epik_amd_ancestral_desc &d, const ancestral_tree &tree, const uint32_t *masks, uint64_t L,
                         uint32_t ghosts, uint32_t num_threads, float *post, uint64_t *dead_sites)
{
    // blocks of sites, so that a thread's work arrays are allocated a few times only
    const uint64_t block = 8, blocks = (L + block - 1) / block;
    std::vector<uint64_t> dead(blocks, 0);
    parallel_for(blocks, num_threads, [&](size_t i) {
        SiteWork w;
        for (uint64_t s = i * block; s < std::min<uint64_t>(L, (i + 1) * block); ++s) dead[i] += one_site(d, tree, masks, L, s, ghosts, post, w);
    });
    uint64_t total = 0;
    for (const uint64_t n : dead) total += n;
    if (dead_sites) *dead_sites = total;
}

// ---- the model side ---------------------------------------------------------------------------------------------------

namespace {

// cyclic Jacobi on the symmetric a[n][n]: eigenvalues on its diagonal, eigenvectors in the columns of v
void jacobi_eigen(std::vector<double> &a, std::vector<double> &v, uint32_t n)
{
    v.assign((size_t)n * n, 0.0);
    for (uint32_t i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = 0; j < n; ++j) (i == j ? diag : off) += a[(size_t)i * n + j] * a[(size_t)i * n + j];
        if (off <= 1e-36 * diag || off == 0.0) break;
        for (uint32_t p = 0; p + 1 < n; ++p)
            for (uint32_t q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (uint32_t k = 0; k < n; ++k) {
                    const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * akp - s * akq, a[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (uint32_t k = 0; k < n; ++k) {
                    const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
                    a[(size_t)p * n + k] = c * apk - s * aqk, a[(size_t)q * n + k] = s * apk + c * aqk;
                }
                for (uint32_t k = 0; k < n; ++k) {
                    const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * vkp - s * vkq, v[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
}

}  // namespace

int model_pmatrices(uint32_t sigma, const double *exchange, const double *pi, const double *times, uint64_t n, double *out,
                    std::string &err)
{
    const uint32_t S = sigma;
    if (S < 2 || S > 64) return invalid(err, "sigma = " + std::to_string(S) + " is outside [2, 64]");
    if (!exchange || !pi || (n && (!times || !out))) return invalid(err, "null argument");
    double total = 0.0;
    for (uint32_t x = 0; x < S; ++x) {
        if (!(pi[x] > 0.0) || !std::isfinite(pi[x])) return invalid(err, "pi[" + std::to_string(x) + "] is not a finite number above 0");
        total += pi[x];
    }
    std::vector<double> f(S), root(S), r((size_t)S * S, 0.0);
    for (uint32_t x = 0; x < S; ++x) f[x] = pi[x] / total, root[x] = std::sqrt(f[x]);
    size_t at = 0;
    for (uint32_t x = 0; x < S; ++x)
        for (uint32_t y = x + 1; y < S; ++y, ++at) {
            if (!(exchange[at] >= 0.0) || !std::isfinite(exchange[at]))
                return invalid(err, "exchangeability " + std::to_string(at) + " is not a finite number that is at least 0");
            r[(size_t)x * S + y] = r[(size_t)y * S + x] = exchange[at];
        }
    // Q[x][y] = r[x][y] f[y], rows summing to 0, scaled to one expected substitution per unit time
    double mu = 0.0;
    for (uint32_t x = 0; x < S; ++x)
        for (uint32_t y = 0; y < S; ++y)
            if (x != y) mu += f[x] * r[(size_t)x * S + y] * f[y];
    if (!(mu > 0.0)) return invalid(err, "every exchangeability is 0: the model has no substitutions");
    std::vector<double> b((size_t)S * S, 0.0), v;
    for (uint32_t x = 0; x < S; ++x) {
        double row = 0.0;
        for (uint32_t y = 0; y < S; ++y)
            if (x != y) {
                b[(size_t)x * S + y] = root[x] * r[(size_t)x * S + y] * root[y] / mu;
                row += r[(size_t)x * S + y] * f[y] / mu;
            }
        b[(size_t)x * S + x] = -row;
    }
    jacobi_eigen(b, v, S);
    std::vector<double> e(S);
    for (uint64_t i = 0; i < n; ++i) {
        const double t = times[i];
        double *P = out + i * S * S;
        if (!(t >= 0.0) || !std::isfinite(t)) return invalid(err, "times[" + std::to_string(i) + "] is not a finite number that is at least 0");
        if (t == 0.0) {
            for (uint32_t x = 0; x < S; ++x)
                for (uint32_t y = 0; y < S; ++y) P[(size_t)x * S + y] = x == y ? 1.0 : 0.0;
            continue;
        }
        for (uint32_t k = 0; k < S; ++k) e[k] = std::exp(std::min(0.0, b[(size_t)k * S + k]) * t);
        for (uint32_t x = 0; x < S; ++x)
            for (uint32_t y = 0; y < S; ++y) {
                double acc = 0.0;
                for (uint32_t k = 0; k < S; ++k) acc += v[(size_t)x * S + k] * e[k] * v[(size_t)y * S + k];
                P[(size_t)x * S + y] = std::max(0.0, acc * root[y] / root[x]);
            }
    }
    return EPIK_AMD_OK;
}

double gamma_p(double a, double x)
{
    if (!(x > 0.0)) return 0.0;
    if (std::isinf(x)) return 1.0;
    const double front = std::exp(a * std::log(x) - x - std::lgamma(a));
    if (x < a + 1.0) {  // the series  x^a e^-x / Gamma(a + 1) * sum of x^n / ((a + 1) .. (a + n))
        double term = 1.0 / a, sum = term;
        for (int n = 1; n < 100000; ++n) {
            term *= x / (a + n);
            sum += term;
            if (term < sum * 1e-17) break;
        }
        return std::min(1.0, front * sum);
    }
    // Q(a, x) by the continued fraction (modified Lentz)
    const double tiny = 1e-300;
    double bb = x + 1.0 - a, c = 1.0 / tiny, dd = 1.0 / bb, h = dd;
    for (int n = 1; n < 100000; ++n) {
        const double an = -(double)n * ((double)n - a);
        bb += 2.0;
        dd = an * dd + bb;
        if (std::fabs(dd) < tiny) dd = tiny;
        c = bb + an / c;
        if (std::fabs(c) < tiny) c = tiny;
        dd = 1.0 / dd;
        const double delta = dd * c;
        h *= delta;
        if (std::fabs(delta - 1.0) < 1e-16) break;
    }
    return std::max(0.0, 1.0 - front * h);
}

double gamma_p_inverse(double a, double p)
{
    if (!(p > 0.0)) return 0.0;
    if (p >= 1.0) return std::numeric_limits<double>::infinity();
    double lo = 0.0, hi = std::max(1.0, a);
    while (gamma_p(a, hi) < p) lo = hi, hi *= 2.0;
    double x = 0.5 * (lo + hi);
    for (int it = 0; it < 400; ++it) {
        const double f = gamma_p(a, x) - p;
        if (f > 0.0) hi = x; else lo = x;
        // a Newton step where it stays inside the bracket, the midpoint otherwise
        const double density = std::exp((a - 1.0) * std::log(x) - x - std::lgamma(a));
        double next = density > 0.0 ? x - f / density : 0.5 * (lo + hi);
        if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
        if (next == x || hi - lo <= 4e-16 * hi) break;
        x = next;
    }
    return x;
}

int model_gamma_rates(double alpha, uint32_t K, double *rates, std::string &err)
{
    if (K < 1 || K > kAncestralMaxCategories) return invalid(err, "K = " + std::to_string(K) + " categories is outside [1, " + std::to_string(kAncestralMaxCategories) + "]");
    if (!(alpha > 0.0) || !std::isfinite(alpha)) return invalid(err, "alpha must be a finite number above 0");
    if (!rates) return invalid(err, "null argument");
    // the mean of X in a quantile bin of Gamma(alpha, rate alpha): K (P(alpha + 1, alpha q_i) - P(alpha + 1, alpha q_(i-1)))
    double below = 0.0, sum = 0.0;
    for (uint32_t i = 1; i <= K; ++i) {
        const double upto = i == K ? 1.0 : gamma_p(alpha + 1.0, gamma_p_inverse(alpha, (double)i / K));
        rates[i - 1] = K * (upto - below);
        sum += rates[i - 1];
        below = upto;
    }
    for (uint32_t i = 0; i < K; ++i) rates[i] *= K / sum;
    return EPIK_AMD_OK;
}

}  // namespace epik_amd
