// taxa_selftest.cpp -- the host taxonomy (taxonomy.cpp) on a hand case and a forged batch, a program of its own for the
// sanitizer build (make sanitize-taxa; tests/test_taxa_cpu.py): the parser with its errors, the labeller with its
// errors, the validation, and the rule -- records and cells -- whose results are checked against the hand values and
// against each other.  Needs no GPU and no libepik_amd.  Exit status 0 and "ok", or 1 and what failed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "taxonomy.hpp"

namespace {

int failures = 0;

void expect(bool ok, const std::string& what)
{
    if (ok) return;
    std::printf("FAILED: %s\n", what.c_str());
    ++failures;
}

const char* kHand =
    "# leaf\ttaxopath\n"
    "A\tBacteria;Proteo;Gamma\n"
    "\n"
    "B\tBacteria; Proteo ;Alpha\n"
    "D\tBacteria;Firmi;Bacilli\n"
    "  # the odd one out\n"
    " E \tArchaea;Eury;Halo\r\n";

uint64_t q_of(double x) { return (uint64_t)std::llrint(x * 1073741824.0); }

void parser_errors()
{
    const struct {
        const char* text;
        const char* begins;
    } cases[] = {{"A\tx;y\nB x;y\n", "line 2:"}, {"A\tx;y\n\n# c\nB\tx;;y\n", "line 4:"}, {"A\tx;y\nB\t\n", "line 2:"},
                 {"A\tx;y;\n", "line 1:"},       {"A\tx\nB\ty\n#\nA\tz\n", "line 4:"},   {"\tx\n", "line 1:"}};
    for (const auto& c : cases) {
        std::istringstream in(c.text);
        epik_amd::taxonomy taxa;
        std::string err;
        expect(epik_amd::parse_taxonomy(in, taxa, err) == EPIK_AMD_ERR_INVALID && err.rfind(c.begins, 0) == 0,
               std::string("parser error ") + c.begins + " got: " + err);
    }
}

void hand_case()
{
    std::istringstream in(kHand);
    epik_amd::taxonomy taxa;
    std::string err;
    expect(epik_amd::parse_taxonomy(in, taxa, err) == 0, "the hand taxonomy parses: " + err);
    const std::vector<uint32_t> want_parent = {1, 2, 9, 4, 8, 7, 7, 8, 9, EPIK_AMD_TREE_NO_PARENT};
    const std::vector<uint32_t> want_first = {0, 0, 0, 3, 3, 5, 6, 5, 3, 0};
    expect(taxa.parent == want_parent && taxa.first == want_first, "the hand taxonomy's ids");
    expect(taxa.path[7] == "Bacteria;Proteo" && taxa.path[9].empty() && taxa.path[0] == "Archaea;Eury;Halo", "the hand taxopaths");
    std::vector<uint32_t> first;
    expect(epik_amd::taxonomy_first(taxa.parent.data(), taxa.num_taxa(), "taxon", first, err) == 0 && first == want_first, "first[] validates");
    const std::vector<uint32_t> tree = {2, 2, 6, 5, 5, 6, EPIK_AMD_TREE_NO_PARENT};
    const std::vector<std::string> names = {"A", "B", "C", "D", "E", "F", "R"};
    std::vector<uint32_t> label;
    expect(epik_amd::label_branches(taxa, tree.data(), names, 7, label, err) == 0, "the hand tree is labelled: " + err);
    expect(label == std::vector<uint32_t>({6, 5, 7, 3, 0, 9, 9}), "the hand labels (F backs off to the root)");
    // labeller errors: a leaf the file lacks; a label that is no leaf
    {
        std::vector<std::string> other = names;
        other[4] = "Z";
        std::vector<uint32_t> l;
        expect(epik_amd::label_branches(taxa, tree.data(), other, 7, l, err) != 0 && err.rfind("leaf Z:", 0) == 0, "a missing leaf is named: " + err);
        std::istringstream more(std::string(kHand) + "C\tBacteria\n");
        epik_amd::taxonomy with_inner;
        expect(epik_amd::parse_taxonomy(more, with_inner, err) == 0, "parses");
        expect(epik_amd::label_branches(with_inner, tree.data(), names, 7, l, err) != 0 && err.rfind("line 8:", 0) == 0, "a label that is no leaf names its line: " + err);
    }
    // validation errors
    {
        const uint32_t bad[] = {2, 3, 3, EPIK_AMD_TREE_NO_PARENT};
        expect(epik_amd::taxonomy_first(bad, 4, "taxon", first, err) != 0 && err.rfind("taxon 2:", 0) == 0, "not post-order: " + err);
        const uint32_t two_roots[] = {2, EPIK_AMD_TREE_NO_PARENT, EPIK_AMD_TREE_NO_PARENT};
        expect(epik_amd::taxonomy_first(two_roots, 3, "taxon", first, err) != 0 && err.rfind("taxon 1:", 0) == 0, "two roots: " + err);
    }
    // three reads, keep 7; slots past n_rows hold garbage
    const uint32_t keep = 7;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<epik_amd_placement> rows(3 * keep, epik_amd_placement{0xffffffffu, 0.0f, nan});
    const auto set = [&](uint32_t i, uint32_t j, uint32_t b, double lwr) { rows[i * keep + j] = epik_amd_placement{b, -1.0f, lwr}; };
    set(0, 0, 0, 0.5), set(0, 1, 1, 0.25), set(0, 2, 3, 0.25);
    set(1, 0, 3, 0.4), set(1, 1, 0, 0.3), set(1, 2, 1, 0.3);
    set(2, 0, 5, 0.7), set(2, 1, 4, 0.3);
    const std::vector<uint32_t> n_rows = {3, 3, 2}, counts(3 * keep, 1);
    std::vector<epik_amd_taxon_record> rec(3);
    epik_amd::taxa_cells cells(1, taxa.num_taxa());
    const uint32_t tau = (uint32_t)std::llrint(0.55 * 1073741824.0);
    epik_amd::taxa_assign(taxa.parent.data(), taxa.num_taxa(), label.data(), 7, keep, rows.data(), n_rows.data(), counts.data(),
                          nullptr, nullptr, 3, tau, rec.data(), &cells);
    expect(rec[0].taxon == 7 && rec[0].taxon_mass_q == (3u << 28) && rec[0].first_taxon == 6 && rec[0].total_q == (1u << 30), "read 0 at .55");
    expect(rec[1].taxon == 7 && rec[1].taxon_mass_q == 2 * q_of(0.3) && rec[1].first_taxon == 3, "read 1 at .55: Proteo, not the best row's");
    expect(rec[2].taxon == 9 && rec[2].taxon_mass_q == (1u << 30) && rec[2].first_taxon == 9, "read 2 at .55: the root");
    expect(cells.totals[0].placed == 3 && cells.assigned[7] == 2 && cells.assigned[9] == 1, "the hand cells");
    const auto clade = epik_amd::clade_sums(cells.direct.data(), first.data(), taxa.num_taxa());
    expect(clade[8] == (1u << 30) + q_of(0.4) + 2 * q_of(0.3) && clade[2] == q_of(0.3), "the hand clade sums");
}

// rows no placement writes, from a small generator: every class, bad rows, n_rows beyond keep, LWRs of 0 and of 1
void forged_batch(uint32_t keep)
{
    const uint32_t T = 101, N = 57, S = 4;
    const uint64_t n = 1500;
    std::vector<uint32_t> parent(T), first;
    parent[0] = parent[1] = 2;  // a caterpillar
    for (uint32_t inner = 2; inner + 2 < T; inner += 2) parent[inner] = parent[inner + 1] = inner + 2;
    parent[T - 1] = EPIK_AMD_TREE_NO_PARENT;
    std::string err;
    expect(epik_amd::taxonomy_first(parent.data(), T, "taxon", first, err) == 0, "the caterpillar validates: " + err);
    uint64_t state = 88172645463325252ull + keep;
    const auto next = [&]() {
        state ^= state << 13, state ^= state >> 7, state ^= state << 17;
        return state;
    };
    std::vector<uint32_t> label(N), n_rows(n), counts(n * keep, 3), weights(n), samples(n);
    for (auto& l : label) l = (uint32_t)(next() % T);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<epik_amd_placement> rows(n * keep);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t kind = (uint32_t)(i % 8);
        n_rows[i] = kind == 6 ? 0u : kind == 7 ? EPIK_AMD_ROWS_COUNTS_TOO_NARROW : kind == 5 ? keep + 5 : 1 + (uint32_t)(next() % keep);
        if (i % 11 == 5) counts[i * keep] = 0;
        weights[i] = i % 13 == 5 ? 0xffffffffu : (uint32_t)(next() % 5);
        samples[i] = i % 97 == 3 ? S + 5 : (uint32_t)(i * S / n);
        const uint32_t live = n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW ? 0u : n_rows[i] < keep ? n_rows[i] : keep;
        for (uint32_t j = 0; j < keep; ++j) {
            epik_amd_placement& r = rows[i * keep + j];
            if (j >= live) {
                r = epik_amd_placement{0xffffffffu, 0.0f, nan};
                continue;
            }
            r.branch = (uint32_t)(next() % N), r.score = -1.0f;
            r.lwr = i % 5 == 2 ? 0.0 : i % 5 == 3 ? 1.0 : (double)(next() % 1000) / 1000.0 / keep;
        }
        if (i % 17 == 3 && live) rows[i * keep + next() % live].branch = N + (uint32_t)(next() % 2);
    }
    for (const uint32_t tau : {(1u << 29) + 1, 1020054733u, 1u << 30}) {
        std::vector<epik_amd_taxon_record> rec(n);
        epik_amd::taxa_cells cells(S, T), again(S, T);
        epik_amd::taxa_assign(parent.data(), T, label.data(), N, keep, rows.data(), n_rows.data(), counts.data(), weights.data(),
                              samples.data(), n, tau, rec.data(), &cells);
        epik_amd::taxa_assign(parent.data(), T, label.data(), N, keep, rows.data(), n_rows.data(), counts.data(), weights.data(),
                              samples.data(), n, tau, nullptr, &again);
        expect(cells.direct == again.direct && cells.assigned == again.assigned && cells.bad_samples == again.bad_samples, "cells with and without records");
        uint64_t classes[5] = {0, 0, 0, 0, 0}, placed = 0, assigned = 0, placed_w = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (rec[i].taxon >= EPIK_AMD_TAXON_NO_MASS) {
                ++classes[0xffffffffu - rec[i].taxon];
                expect(rec[i].taxon_mass_q == 0 && rec[i].first_taxon == 0 && rec[i].total_q == 0, "a class record is otherwise zero");
                continue;
            }
            ++placed;
            expect(rec[i].taxon < T && rec[i].first_taxon < T && rec[i].taxon_mass_q <= rec[i].total_q, "a placed record is in range");
            expect(first[rec[i].taxon] <= rec[i].first_taxon || rec[i].taxon_mass_q < rec[i].total_q || tau < (1u << 30), "all of the mass: every row inside");
            if (tau == (1u << 30)) expect(rec[i].taxon_mass_q == rec[i].total_q, "all of the mass is all of it");
        }
        for (uint32_t s = 0; s < S; ++s) placed_w += cells.totals[s].placed;
        for (const uint64_t a : cells.assigned) assigned += a;
        expect(placed > n / 4 && classes[0] && classes[1] && classes[2] && classes[3] && classes[4], "every class occurs");
        expect(assigned == placed_w && cells.bad_samples > 2, "assigned sums to placed");
    }
}

}  // namespace

int main()
{
    parser_errors();
    hand_case();
    for (const uint32_t keep : {1u, 7u, 64u}) forged_batch(keep);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
