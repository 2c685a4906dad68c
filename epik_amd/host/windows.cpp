#include "windows.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <exception>
#include <fstream>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "cohort.hpp"
#include "confidence.hpp"
#include "placer.hpp"
#include "seq_record.hpp"

namespace epik_amd {

namespace {

/// A whole number in [lo, hi], or the refusal `what`
uint64_t whole_number(const std::string& text, uint64_t lo, uint64_t hi, const std::string& what)
{
    size_t used = 0;
    unsigned long long value = 0;
    try {
        if (text.empty() || text[0] == '-' || text[0] == '+') throw std::invalid_argument(text);
        value = std::stoull(text, &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (used != text.size() || used == 0 || value < lo || value > hi) throw std::runtime_error(what + ", not '" + text + "'");
    return value;
}

std::string base_of(const std::string& file)
{
    const auto slash = file.find_last_of('/');
    return slash == std::string::npos ? file : file.substr(slash + 1);
}

std::string in_dir(const std::string& prefix, const std::string& query_file, const std::string& output_dir)
{
    std::string dir = output_dir;
    if (!dir.empty() && dir.back() != '/') dir.push_back('/');
    return dir + prefix + base_of(query_file) + ".tsv";
}

const char* status_name(uint32_t call)
{
    switch (call) {
    case EPIK_AMD_WINDOW_TOO_NARROW: return "too_narrow";
    case EPIK_AMD_WINDOW_TOO_SHORT: return "too_short";
    case EPIK_AMD_WINDOW_NO_HIT: return "no_hit";
    case EPIK_AMD_WINDOW_BAD_ROW: return "bad_row";
    case EPIK_AMD_WINDOW_NO_MASS: return "no_mass";
    default: return "ambiguous";
    }
}

std::string call_name(uint32_t call, const windows_plan& plan)
{
    return call < EPIK_AMD_WINDOW_AMBIGUOUS && call < plan.group_paths.size() ? plan.group_paths[call] : status_name(call);
}

std::string g17(double x)
{
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", x);
    return buf;
}

void span_of(uint64_t length, const windows_plan& plan, uint64_t w, uint64_t& begin, uint64_t& end)
{
    begin = end = 0;
    (void)epik_amd_window_span(length, plan.window, plan.step, w, &begin, &end);
}

}  // namespace

windows_plan parse_windows_options(const options& parsed)
{
    windows_plan plan;
    plan.with_windows = parsed.has("windows");
    for (const char* flag : {"window-step", "window-mass", "window-groups", "window-rank", "windows-per-window"})
        if (parsed.has(flag) && !plan.with_windows) throw std::runtime_error(std::string("--") + flag + " needs --windows");
    if (!plan.with_windows) return plan;
    if (!parsed.has("window-groups")) throw std::runtime_error("--windows needs --window-groups");
    for (const char* flag : {"mates", "translate", "profile", "profile-only", "assign", "taxonomy", "cohort"})
        if (parsed.has(flag)) throw std::runtime_error(std::string("--windows does not work with --") + flag);
    if (std::stoul(parsed.get("db-shard", "1")) > 1) throw std::runtime_error("--windows does not work with --db-shard > 1");
    plan.window = (uint32_t)whole_number(parsed.require("windows"), 1, 0x7fffffffull, "--windows must be a whole number in [1, 2^31)");
    const uint32_t default_step = std::max<uint32_t>(1, plan.window / 4);
    plan.step = parsed.has("window-step")
                    ? (uint32_t)whole_number(parsed.require("window-step"), 1, plan.window,
                                             "--window-step must be a whole number in [1, " + std::to_string(plan.window) + "]")
                    : default_step;
    plan.rank = (uint32_t)whole_number(parsed.get("window-rank", "1"), 1, 0xffffffffull, "--window-rank must be a whole number from 1 up");
    {
        size_t used = 0;
        const auto text = parsed.get("window-mass", "0.8");
        double share = -1.0;
        try {
            share = std::stod(text, &used);
        } catch (const std::exception&) {
            used = 0;
        }
        if (used != text.size() || used == 0 || !(share > 0.5) || !(share <= 1.0))
            throw std::runtime_error("--window-mass must be a number in (0.5, 1], not '" + text + "'");
        plan.tau_q = assign_tau_q(share);
        if (plan.tau_q <= (1u << 29) || plan.tau_q > (1u << 30))
            throw std::runtime_error("--window-mass must be a number in (0.5, 1], not '" + text + "'");
    }
    plan.per_window = parsed.has("windows-per-window");
    plan.groups_file = parsed.require("window-groups");
    return plan;
}

void windows_plan::read_inputs()
{
    if (!with_windows) return;
    std::ifstream in(groups_file, std::ios::binary);
    if (!in) throw std::runtime_error("Could not open the groups file " + groups_file);
    std::string err;
    if (parse_taxonomy(in, taxa, err) != 0) throw std::runtime_error(groups_file + ": " + err);
}

void windows_plan::label(const uint32_t* parent, const std::vector<std::string>& names, uint32_t n)
{
    std::vector<uint32_t> labels, group_taxa;
    std::string err;
    if (label_branches(taxa, parent, names, n, labels, err) != 0) throw std::runtime_error(groups_file + ": " + err);
    groups_at_rank(taxa, labels, rank, group, group_taxa);
    group_paths.clear();
    for (const uint32_t t : group_taxa) group_paths.push_back(taxa.path[t]);
}

std::string format_windows_header(const windows_plan& plan, uint64_t records)
{
    std::string out = "# epik_amd windows v1\twindow=" + std::to_string(plan.window) + "\tstep=" + std::to_string(plan.step) +
                      "\ttau_q=" + std::to_string(plan.tau_q) + "\tgroups=" + std::to_string(plan.group_paths.size()) +
                      "\trank=" + std::to_string(plan.rank) + "\trecords=" + std::to_string(records) + "\n";
    for (size_t g = 0; g < plan.group_paths.size(); ++g) out += "# group\t" + std::to_string(g) + "\t" + plan.group_paths[g] + "\n";
    return out + "name\tsegment\tstart\tend\twindows\tcall\tsupport\n";
}

std::string format_window_segments(const std::string& name, uint64_t length, const windows_plan& plan,
                                   const epik_amd_window_segment* segments, uint32_t n_segments)
{
    std::string out;
    for (uint32_t s = 0; s < n_segments; ++s) {
        const auto& seg = segments[s];
        uint64_t start = 0, end = 0, other = 0;
        span_of(length, plan, seg.first_window, start, other);
        span_of(length, plan, (uint64_t)seg.first_window + seg.num_windows - 1, other, end);
        const bool called = seg.call < EPIK_AMD_WINDOW_AMBIGUOUS;
        out += name + "\t" + std::to_string(s) + "\t" + std::to_string(start) + "\t" + std::to_string(end) + "\t" +
               std::to_string(seg.num_windows) + "\t" + call_name(seg.call, plan) + "\t" +
               (called ? g17((double)seg.call_mass / (double)seg.total) : std::string("NA")) + "\n";
    }
    return out;
}

std::string format_window_breakpoints(const std::string& name, uint64_t length, const windows_plan& plan,
                                      const epik_amd_window_segment* segments, uint32_t n_segments, uint64_t* count)
{
    std::string out;
    const epik_amd_window_segment* left = nullptr;
    for (uint32_t s = 0; s < n_segments; ++s) {
        const auto& seg = segments[s];
        if (seg.call >= EPIK_AMD_WINDOW_AMBIGUOUS) continue;  // (uncalled segments between two called ones are skipped)
        if (left && left->call != seg.call) {
            uint64_t from = 0, to = 0, other = 0;
            span_of(length, plan, (uint64_t)left->first_window + left->num_windows - 1, from, other);
            span_of(length, plan, seg.first_window, other, to);
            out += name + "\t" + call_name(left->call, plan) + "\t" + call_name(seg.call, plan) + "\t" + std::to_string(from) + "\t" +
                   std::to_string(to) + "\n";
            if (count) ++*count;
        }
        left = &seg;
    }
    return out;
}

windows_report run_windows(placer& placer, const windows_plan& plan, uint32_t strand_mode, const std::string& query_file,
                           const std::string& output_dir, size_t batch_size, size_t num_threads)
{
    windows_report report;
    report.windows_file = in_dir("windows_", query_file, output_dir);
    report.breakpoints_file = in_dir("windows_breakpoints_", query_file, output_dir);
    if (plan.per_window) report.all_file = in_dir("windows_all_", query_file, output_dir);

    // The reader keeps the file mapped; the batches are read up front (views, no copies), dealt to the callers, and every
    // batch's lines are kept until all are there: the files are written once, in input order.
    io::batch_fasta reader(query_file, std::max<size_t>(batch_size, 1));
    std::vector<std::vector<seq_record>> batches;
    for (;;) {
        auto batch = reader.next_batch();
        if (batch.empty()) break;
        batches.push_back(std::move(batch));
    }
    struct lines {
        std::string segments, breakpoints, all;
        uint64_t windows = 0, n_segments = 0, n_breakpoints = 0;
    };
    std::vector<lines> done(batches.size());
    const size_t callers = std::max<size_t>(1, std::min<size_t>({placer.device_count() * 2, std::max<size_t>(num_threads, placer.device_count()), batches.size()}));
    std::atomic<size_t> next{0};
    std::vector<std::exception_ptr> errors(callers);
    std::vector<std::mutex> device_mutex(placer.device_count());
    const auto work = [&](size_t caller) {
        try {
            const size_t device = caller % placer.device_count();
            for (size_t b = next++; b < batches.size(); b = next++) {
                const auto& batch = batches[b];
                placer::window_batch painted;
                {
                    std::lock_guard<std::mutex> lock(device_mutex[device]);  // (a handle serves one call at a time)
                    painted = placer.paint_windows(batch, device, plan.window, plan.step, strand_mode, plan.group, plan.tau_q, plan.per_window);
                }
                auto& out = done[b];
                for (size_t i = 0; i < batch.size(); ++i) {
                    const std::string name(batch[i].header());
                    const uint64_t length = batch[i].sequence().size(), v0 = painted.win_offsets[i], v1 = painted.win_offsets[i + 1];
                    out.segments += format_window_segments(name, length, plan, painted.segments.data() + v0, painted.n_segments[i]);
                    out.breakpoints += format_window_breakpoints(name, length, plan, painted.segments.data() + v0, painted.n_segments[i], &out.n_breakpoints);
                    out.windows += v1 - v0, out.n_segments += painted.n_segments[i];
                    if (!plan.per_window) continue;
                    for (uint64_t v = v0; v < v1; ++v) {
                        uint64_t begin = 0, end = 0;
                        span_of(length, plan, v - v0, begin, end);
                        const auto& rec = painted.records[v];
                        const bool called = rec.call < EPIK_AMD_WINDOW_AMBIGUOUS;
                        const bool has_rows = painted.n_rows[v] != 0 && painted.n_rows[v] != EPIK_AMD_ROWS_COUNTS_TOO_NARROW;
                        out.all += name + "\t" + std::to_string(v - v0) + "\t" + std::to_string(begin) + "\t" + std::to_string(end) + "\t" +
                                   (painted.strand[v] ? "-" : "+") + "\t" + call_name(rec.call, plan) + "\t" +
                                   (called ? g17((double)rec.call_mass_q / (double)rec.total_q) : std::string("NA")) + "\t" +
                                   (has_rows ? std::to_string(painted.best[v].branch) : std::string("NA")) + "\t" +
                                   (has_rows ? g17(painted.best[v].lwr) : std::string("NA")) + "\n";
                    }
                }
            }
        } catch (...) {
            errors[caller] = std::current_exception();
            next = batches.size();
        }
    };
    std::vector<std::thread> threads;
    for (size_t c = 1; c < callers; ++c) threads.emplace_back(work, c);
    work(0);
    for (auto& t : threads) t.join();
    for (const auto& error : errors)
        if (error) std::rethrow_exception(error);

    for (const auto& batch : batches) report.records += batch.size();
    std::string segments = format_windows_header(plan, report.records), breakpoints = "name\tleft\tright\tfrom\tto\n";
    std::string all = "name\twindow\tstart\tend\tstrand\tcall\tshare\tbest_edge_num\tbest_lwr\n";
    for (auto& out : done) {
        segments += out.segments, breakpoints += out.breakpoints;
        if (plan.per_window) all += out.all;
        report.windows += out.windows, report.segments += out.n_segments, report.breakpoints += out.n_breakpoints;
        out = lines{};
    }
    write_through_part(report.windows_file, segments);
    write_through_part(report.breakpoints_file, breakpoints);
    if (plan.per_window) write_through_part(report.all_file, all);
    return report;
}

}  // namespace epik_amd
