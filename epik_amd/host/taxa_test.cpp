// taxa_test.cpp -- the host taxonomy (taxonomy.cpp) driven from files, for tests/test_taxa_cpu.py; needs no GPU and no
// libepik_amd.
//   taxa_test labels <taxonomy.tsv> <tree.bin> <out.bin>   parses the file and labels the tree.  tree.bin: uint64 N;
//                                                          uint32 parent[N]; N names, each uint32 length + bytes.
//                                                          out.bin: uint64 T; uint32 taxon_parent[T]; uint32 first[T];
//                                                          uint32 label[N]; T taxopaths, each uint32 length + bytes.
//                                                          An error goes to stdout, exit status 1.
//   taxa_test groups <taxonomy.tsv> <tree.bin> <depth> <out.bin>  the groups painting by windows calls at that depth
//                                                          (groups_at_rank): uint64 G; uint32 group[N]; uint32 group_taxa[G]
//   taxa_test records <tau_q> <in.bin> <out.bin>           epik_amd_taxon_record [n]
//   taxa_test cells <tau_q> <in.bin> <out.bin>             uint64 direct[S][T], assigned[S][T], totals[S][6], bad_samples
//   taxa_test files <tau_q> <in.bin> <taxonomy.tsv> <prefix>  the three files of that batch, every read named read_<i> and
//                                                          sample s named sample_<s>: <prefix>taxa.tsv (sample 0),
//                                                          <prefix>taxa_reads.tsv, <prefix>cohort_taxa.tsv
// in.bin holds, little endian: uint64 n, keep, N, T, S; epik_amd_placement rows[n][keep]; uint32 n_rows[n]; uint32
// kmer_counts[n][keep]; uint32 weights[n]; uint32 samples[n]; uint32 taxon_parent[T]; uint32 label[N].
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "taxonomy.hpp"

namespace {

template <typename T>
std::vector<T> read_array(std::ifstream& in, size_t count)
{
    std::vector<T> v(count);
    in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    if (!in) throw std::runtime_error("input file too short");
    return v;
}

template <typename T>
void write_array(std::ofstream& out, const T* data, size_t count)
{
    out.write(reinterpret_cast<const char*>(data), (std::streamsize)(count * sizeof(T)));
}

int labels(const char* taxonomy_path, const char* tree_path, const char* out_path, const char* depth = nullptr)
{
    std::ifstream text(taxonomy_path);
    if (!text) throw std::runtime_error(std::string("cannot open ") + taxonomy_path);
    epik_amd::taxonomy taxa;
    std::string err;
    if (epik_amd::parse_taxonomy(text, taxa, err) != 0) {
        std::cout << err << "\n";
        return 1;
    }
    std::ifstream in(tree_path, std::ios::binary);
    if (!in) throw std::runtime_error(std::string("cannot open ") + tree_path);
    const uint64_t n = read_array<uint64_t>(in, 1)[0];
    const auto parent = read_array<uint32_t>(in, n);
    std::vector<std::string> names(n);
    for (auto& name : names) {
        const uint32_t length = read_array<uint32_t>(in, 1)[0];
        const auto bytes = read_array<char>(in, length);
        name.assign(bytes.begin(), bytes.end());
    }
    std::vector<uint32_t> label;
    if (epik_amd::label_branches(taxa, parent.data(), names, (uint32_t)n, label, err) != 0) {
        std::cout << err << "\n";
        return 1;
    }
    std::vector<uint32_t> first;
    if (epik_amd::taxonomy_first(taxa.parent.data(), taxa.num_taxa(), "taxon", first, err) != 0 || first != taxa.first)
        throw std::runtime_error("the parser's taxonomy does not validate: " + err);
    std::ofstream out(out_path, std::ios::binary);
    if (depth) {
        std::vector<uint32_t> group, group_taxa;
        epik_amd::groups_at_rank(taxa, label, (uint32_t)std::stoul(depth), group, group_taxa);
        const uint64_t G = group_taxa.size();
        write_array(out, &G, 1);
        write_array(out, group.data(), group.size());
        write_array(out, group_taxa.data(), group_taxa.size());
        if (!out) throw std::runtime_error(std::string("cannot write ") + out_path);
        return 0;
    }
    const uint64_t T = taxa.num_taxa();
    write_array(out, &T, 1);
    write_array(out, taxa.parent.data(), T);
    write_array(out, taxa.first.data(), T);
    write_array(out, label.data(), label.size());
    for (const auto& path : taxa.path) {
        const uint32_t length = (uint32_t)path.size();
        write_array(out, &length, 1);
        write_array(out, path.data(), path.size());
    }
    if (!out) throw std::runtime_error(std::string("cannot write ") + out_path);
    return 0;
}

int assign(bool want_records, const char* tau, const char* in_path, const char* out_path)
{
    std::ifstream in(in_path, std::ios::binary);
    if (!in) throw std::runtime_error(std::string("cannot open ") + in_path);
    const auto head = read_array<uint64_t>(in, 5);
    const uint64_t n = head[0], keep = head[1], N = head[2], T = head[3], S = head[4];
    const auto rows = read_array<epik_amd_placement>(in, n * keep);
    const auto n_rows = read_array<uint32_t>(in, n);
    const auto counts = read_array<uint32_t>(in, n * keep);
    const auto weights = read_array<uint32_t>(in, n);
    const auto samples = read_array<uint32_t>(in, n);
    const auto parent = read_array<uint32_t>(in, T);
    const auto label = read_array<uint32_t>(in, N);
    std::vector<uint32_t> first;
    std::string err;
    if (epik_amd::taxonomy_first(parent.data(), (uint32_t)T, "taxon", first, err) != 0) {
        std::cout << err << "\n";
        return 1;
    }
    std::vector<epik_amd_taxon_record> records(n);
    epik_amd::taxa_cells cells((uint32_t)S, (uint32_t)T);
    epik_amd::taxa_assign(parent.data(), (uint32_t)T, label.data(), (uint32_t)N, (uint32_t)keep, rows.data(),
                          n_rows.data(), counts.data(), weights.data(), samples.data(), n, (uint32_t)std::stoul(tau),
                          want_records ? records.data() : nullptr, want_records ? nullptr : &cells);
    std::ofstream out(out_path, std::ios::binary);
    if (want_records) {
        write_array(out, records.data(), records.size());
    } else {
        write_array(out, cells.direct.data(), cells.direct.size());
        write_array(out, cells.assigned.data(), cells.assigned.size());
        write_array(out, cells.totals.data(), cells.totals.size());
        write_array(out, &cells.bad_samples, 1);
    }
    if (!out) throw std::runtime_error(std::string("cannot write ") + out_path);
    return 0;
}

int files(const char* tau, const char* in_path, const char* taxonomy_path, const std::string& prefix)
{
    std::ifstream text(taxonomy_path);
    if (!text) throw std::runtime_error(std::string("cannot open ") + taxonomy_path);
    epik_amd::taxonomy taxa;
    std::string err;
    if (epik_amd::parse_taxonomy(text, taxa, err) != 0) throw std::runtime_error(err);
    std::ifstream in(in_path, std::ios::binary);
    if (!in) throw std::runtime_error(std::string("cannot open ") + in_path);
    const auto head = read_array<uint64_t>(in, 5);
    const uint64_t n = head[0], keep = head[1], N = head[2], T = head[3], S = head[4];
    const auto rows = read_array<epik_amd_placement>(in, n * keep);
    const auto n_rows = read_array<uint32_t>(in, n);
    const auto counts = read_array<uint32_t>(in, n * keep);
    const auto weights = read_array<uint32_t>(in, n);
    const auto samples = read_array<uint32_t>(in, n);
    const auto parent = read_array<uint32_t>(in, T);
    const auto label = read_array<uint32_t>(in, N);
    if (parent != taxa.parent) throw std::runtime_error("the taxonomy file and the input's taxon_parent differ");
    const uint32_t tau_q = (uint32_t)std::stoul(tau);
    std::vector<epik_amd_taxon_record> records(n);
    epik_amd::taxa_cells cells((uint32_t)S, (uint32_t)T);
    epik_amd::taxa_assign(parent.data(), (uint32_t)T, label.data(), (uint32_t)N, (uint32_t)keep, rows.data(), n_rows.data(), counts.data(),
                          weights.data(), samples.data(), n, tau_q, records.data(), &cells);
    std::ofstream one(prefix + "taxa.tsv", std::ios::binary), reads(prefix + "taxa_reads.tsv", std::ios::binary),
        cohort(prefix + "cohort_taxa.tsv", std::ios::binary);
    one << epik_amd::format_taxa_tsv(cells, 0, taxa, tau_q);
    reads << epik_amd::format_taxa_reads_header(tau_q, n);
    for (uint64_t i = 0; i < n; ++i) reads << epik_amd::format_taxa_reads_line("read_" + std::to_string(i), records[i], taxa);
    std::vector<std::string> names;
    for (uint64_t s = 0; s < S; ++s) names.push_back("sample_" + std::to_string(s));
    cohort << epik_amd::format_cohort_taxa_tsv(names, cells, taxa, tau_q);
    if (!one || !reads || !cohort) throw std::runtime_error("cannot write " + prefix + "*.tsv");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    try {
        if (argc == 5 && std::strcmp(argv[1], "labels") == 0) return labels(argv[2], argv[3], argv[4]);
        if (argc == 6 && std::strcmp(argv[1], "groups") == 0) return labels(argv[2], argv[3], argv[5], argv[4]);
        if (argc == 5 && std::strcmp(argv[1], "records") == 0) return assign(true, argv[2], argv[3], argv[4]);
        if (argc == 5 && std::strcmp(argv[1], "cells") == 0) return assign(false, argv[2], argv[3], argv[4]);
        if (argc == 6 && std::strcmp(argv[1], "files") == 0) return files(argv[2], argv[3], argv[4], argv[5]);
        std::cerr << "usage: taxa_test labels <taxonomy.tsv> <tree.bin> <out.bin> | records|cells <tau_q> <in.bin> <out.bin> |\n"
                     "       taxa_test groups <taxonomy.tsv> <tree.bin> <depth> <out.bin> |\n"
                     "       taxa_test files <tau_q> <in.bin> <taxonomy.tsv> <prefix>\n";
        return 2;
    } catch (const std::exception& e) {
        std::cerr << "taxa_test: " << e.what() << "\n";
        return 3;
    }
}
