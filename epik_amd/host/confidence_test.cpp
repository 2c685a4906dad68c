// confidence_test.cpp -- the host mirror of the placement confidence (confidence.cpp) driven from files, for
// tests/test_assign_cpu.py; needs no GPU and no libepik_amd.
//   confidence_test tree <newick>                  the rule's tree of a Newick string: a line "id parent first depth mid" per node
//   confidence_test validate <tree.bin>            "ok", or the message of the validation error (exit code 1)
//   confidence_test records <tau_q> <in.bin> <out.bin>            the records of the reads of the input, as they lie in memory
//   confidence_test tsv <tau_q> <in.bin> <assign.tsv> <clades.tsv>  both files of --assign: read i is the input record
//                                                  "read_<i>", and counts weights[i] records in the clade sums
// tree.bin, little endian: uint64 num_branches; uint32 parent[num_branches]; double branch_length[num_branches].
// in.bin: uint64 n, keep, num_branches; epik_amd_placement rows[n][keep]; uint32 n_rows[n]; uint32 kmer_counts[n][keep];
// uint32 weights[n]; uint32 parent[num_branches]; double branch_length[num_branches].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "confidence.hpp"

namespace {

template <typename T>
std::vector<T> read_array(std::ifstream& in, size_t count)
{
    std::vector<T> v(count);
    in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    if (!in) throw std::runtime_error("input file too short");
    return v;
}

std::ifstream open_input(const char* path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error(std::string("cannot open ") + path);
    return in;
}

struct batch {
    uint64_t n = 0, keep = 0;
    std::vector<epik_amd_placement> rows;
    std::vector<uint32_t> n_rows, counts, weights;
    std::vector<epik_amd_confidence> records;
};

batch run(const char* path, uint32_t tau_q, epik_amd::confidence_tree*& tree)
{
    auto in = open_input(path);
    const auto head = read_array<uint64_t>(in, 3);
    batch b;
    b.n = head[0], b.keep = head[1];
    b.rows = read_array<epik_amd_placement>(in, b.n * b.keep);
    b.n_rows = read_array<uint32_t>(in, b.n);
    b.counts = read_array<uint32_t>(in, b.n * b.keep);
    b.weights = read_array<uint32_t>(in, b.n);
    auto parent = read_array<uint32_t>(in, head[2]);
    auto length = read_array<double>(in, head[2]);
    tree = new epik_amd::confidence_tree(std::move(parent), std::move(length));
    b.records.resize(b.n);
    epik_amd::confidence_rows(*tree, b.rows.data(), b.n_rows.data(), b.counts.data(), b.n, (uint32_t)b.keep, tau_q, b.records.data());
    return b;
}

}  // namespace

int main(int argc, char** argv)
{
    try {
        const std::string mode = argc >= 2 ? argv[1] : "";
        if (mode == "tree" && argc == 3) {
            const auto tree = epik_amd::io::parse_newick(argv[2]);
            const epik_amd::confidence_tree t(tree);
            for (size_t b = 0; b < t.num_branches(); ++b)
                std::printf("%zu %lld %u %.17g %.17g\n", b, t.parent[b] == EPIK_AMD_TREE_NO_PARENT ? -1ll : (long long)t.parent[b],
                            t.first[b], t.depth[b], t.mid[b]);
            return 0;
        }
        if (mode == "validate" && argc == 3) {
            auto in = open_input(argv[2]);
            const uint64_t n = read_array<uint64_t>(in, 1)[0];
            auto parent = read_array<uint32_t>(in, n);
            auto length = read_array<double>(in, n);
            try {
                const epik_amd::confidence_tree t(std::move(parent), std::move(length));
            } catch (const std::runtime_error& error) {
                std::cout << error.what() << std::endl;
                return 1;
            }
            std::cout << "ok" << std::endl;
            return 0;
        }
        if (mode == "records" && argc == 5) {
            epik_amd::confidence_tree* tree = nullptr;
            const batch b = run(argv[3], (uint32_t)std::strtoul(argv[2], nullptr, 10), tree);
            std::ofstream out(argv[4], std::ios::binary);
            out.write(reinterpret_cast<const char*>(b.records.data()), (std::streamsize)(b.n * sizeof(epik_amd_confidence)));
            out.close();
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[4]);
            delete tree;
            return 0;
        }
        if (mode == "tsv" && argc == 6) {
            const auto tau_q = (uint32_t)std::strtoul(argv[2], nullptr, 10);
            epik_amd::confidence_tree* tree = nullptr;
            const batch b = run(argv[3], tau_q, tree);
            epik_amd::assign_summary summary(tree->num_branches());
            std::string text = epik_amd::format_assign_header(tau_q, b.n);
            for (uint64_t i = 0; i < b.n; ++i) {
                text += epik_amd::format_assign_line("read_" + std::to_string(i), b.records[i], *tree);
                summary.add(b.records[i], b.weights[i]);
            }
            epik_amd::write_text_file(argv[4], text);
            epik_amd::write_text_file(argv[5], epik_amd::format_assign_clades_tsv(summary, *tree, tau_q));
            delete tree;
            return 0;
        }
        std::cerr << "usage: confidence_test tree <newick> | validate <tree.bin> | records <tau_q> <in.bin> <out.bin> | "
                     "tsv <tau_q> <in.bin> <assign.tsv> <clades.tsv>\n";
        return 2;
    } catch (const std::exception& error) {
        std::cerr << "Error: " << error.what() << std::endl;
        return 1;
    }
}
