// windows.hpp -- long sequences painted by windows in the drivers (include/epik_amd.h: epik_amd_window_span,
// epik_amd_placer_paint_windows): the options of --windows, the groups read from --window-groups, the run over the
// query and the three files.  epik_amd/windows.py formats the same bytes.
#ifndef EPIK_AMD_HOST_WINDOWS_HPP
#define EPIK_AMD_HOST_WINDOWS_HPP
#include <cstdint>
#include <string>
#include <vector>

#include "cohort_run.hpp"
#include "epik_amd.h"
#include "taxonomy.hpp"

namespace epik_amd {

class placer;

/// What --windows and the flags that depend on it ask for
struct windows_plan {
    bool with_windows = false, per_window = false;
    uint32_t window = 0, step = 0, tau_q = 0, rank = 1;
    std::string groups_file;
    taxonomy taxa;                          ///< of --window-groups
    std::vector<uint32_t> group;            ///< [N]: the group of every branch, or EPIK_AMD_WINDOW_NO_GROUP
    std::vector<std::string> group_paths;   ///< the taxopath of every group

    /// Reads the taxonomy file of --window-groups: every error of it, named by its line, before the database or a device is
    void read_inputs();
    /// The groups, at the plan's rank, of the branches of the tree parent[n] whose leaves are named names[b]
    void label(const uint32_t* parent, const std::vector<std::string>& names, uint32_t n);
};

/// The options checked, in the driver's words, before anything is opened
windows_plan parse_windows_options(const options& parsed);

/// What a run wrote
struct windows_report {
    uint64_t records = 0, windows = 0, segments = 0, breakpoints = 0;
    std::string windows_file, breakpoints_file, all_file;
};

/// The whole query painted: batches of `batch_size` records dealt to the placer's devices in turn, `num_threads` callers
/// at the most; the files hold the records in input order whatever the devices, the threads and the batch size.
windows_report run_windows(placer& placer, const windows_plan& plan, uint32_t strand_mode, const std::string& query_file,
                           const std::string& output_dir, size_t batch_size, size_t num_threads);

/// The first lines of windows_<input>.tsv, up to the column names
std::string format_windows_header(const windows_plan& plan, uint64_t records);
/// The lines of one record: its segments, its breakpoints
std::string format_window_segments(const std::string& name, uint64_t length, const windows_plan& plan,
                                   const epik_amd_window_segment* segments, uint32_t n_segments);
std::string format_window_breakpoints(const std::string& name, uint64_t length, const windows_plan& plan,
                                      const epik_amd_window_segment* segments, uint32_t n_segments, uint64_t* count = nullptr);

}  // namespace epik_amd
#endif
