// profile_test.cpp -- the host profile (profile.cpp) driven from files, for tests/test_profile_cpu.py; needs no GPU
// and no libepik_amd.
//   profile_test q <bits>...                  q() of the doubles with these bit patterns (hex), one result a line
//   profile_test tsv <out.tsv> <in.bin>...    the profile of every input, merged, as the TSV the drivers write
// An input holds, little endian: uint64 n, keep, num_branches; epik_amd_placement rows[n][keep]; uint32 n_rows[n];
// uint32 kmer_counts[n][keep]; uint32 weights[n]; uint64 subtree_num_nodes[num_branches].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "profile.hpp"

namespace {

template <typename T>
std::vector<T> read_array(std::ifstream& in, size_t count)
{
    std::vector<T> v(count);
    in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    if (!in) throw std::runtime_error("input file too short");
    return v;
}

}  // namespace

int main(int argc, char** argv)
{
    try {
        if (argc >= 2 && std::strcmp(argv[1], "q") == 0) {
            for (int i = 2; i < argc; ++i) {
                const uint64_t bits = std::strtoull(argv[i], nullptr, 16);
                double x;
                std::memcpy(&x, &bits, sizeof x);
                std::cout << epik_amd::profile_q(x) << '\n';
            }
            return 0;
        }
        if (argc >= 4 && std::strcmp(argv[1], "tsv") == 0) {
            epik_amd::sample_profile total;
            std::vector<size_t> subtree;
            for (int i = 3; i < argc; ++i) {
                std::ifstream in(argv[i], std::ios::binary);
                if (!in) throw std::runtime_error(std::string("cannot open ") + argv[i]);
                const auto head = read_array<uint64_t>(in, 3);
                const uint64_t n = head[0], keep = head[1], branches = head[2];
                const auto rows = read_array<epik_amd_placement>(in, n * keep);
                const auto n_rows = read_array<uint32_t>(in, n);
                const auto counts = read_array<uint32_t>(in, n * keep);
                const auto weights = read_array<uint32_t>(in, n);
                const auto nodes = read_array<uint64_t>(in, branches);
                epik_amd::sample_profile part(branches);
                part.add_rows(rows.data(), n_rows.data(), counts.data(), weights.data(), n, (uint32_t)keep);
                if (i == 3) {
                    total = epik_amd::sample_profile(branches);
                    subtree.assign(nodes.begin(), nodes.end());
                } else if (branches != total.num_branches()) {
                    throw std::runtime_error("inputs of different trees");
                }
                total.merge(part);
            }
            epik_amd::write_profile_tsv(argv[2], total, subtree);
            return 0;
        }
        std::cerr << "usage: profile_test q <bits>... | tsv <out.tsv> <in.bin>...\n";
        return 2;
    } catch (const std::exception& error) {
        std::cerr << "Error: " << error.what() << std::endl;
        return 1;
    }
}
