/*
 * epik_amd.h -- C ABI of the MI355X placement engine (libepik_amd.so).
 *
 * This is the drop-in boundary for EPIK's one hot path, the per-read loop of
 * `epik::placer` (reference: epik/include/epik/place.h:81-140,
 * epik/src/epik/place.cpp:201-440).  The reference has no FFI layer; the
 * narrowest seam the path sits behind is the C++ class `epik::placer`:
 *
 *     placer(const i2l::phylo_kmer_db&, const i2l::phylo_tree&,
 *            size_t keep_at_most, double keep_factor, size_t max_threads);   place.h:94-95
 *     placed_collection place(const std::vector<i2l::seq_record>&, size_t);  place.h:103
 *
 * Each entry point below names the reference interface it replaces.  Plain
 * pointers and sizes only; no C++ or torch types cross the boundary; no
 * exception crosses it either (the reference throws std::runtime_error,
 * place.cpp:104-108,430-433; here every call returns a status code and
 * epik_amd_last_error() holds the message).
 *
 * There is no CPU fallback: every entry point that computes fails with
 * EPIK_AMD_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef EPIK_AMD_H
#define EPIK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPIK_AMD_ABI_VERSION 3

enum epik_amd_status {
    EPIK_AMD_OK = 0,
    EPIK_AMD_ERR_INVALID = 1,   /* bad argument / inconsistent database */
    EPIK_AMD_ERR_NO_DEVICE = 2, /* no usable HIP device (no CPU fallback exists) */
    EPIK_AMD_ERR_HIP = 3,       /* HIP runtime error, see epik_amd_last_error() */
    EPIK_AMD_ERR_UNSUPPORTED = 4 /* configuration outside what the kernels cover */
};

/* i2l::pkdb_value {branch, score}: one phylo-k-mer posting (main.cpp:257,
 * place.cpp:358).  branch = post-order node id, score = log10 probability. */
typedef struct {
    uint32_t branch;
    float score;
} epik_amd_pkdb_value;

/* One reported placement: the fields of epik::impl::placement computed on the
 * hot path (place.h:45-56: branch_id, score, weight_ratio).  distal_length and
 * pendant_length are per-branch constants the host joins (place.cpp:435-437). */
typedef struct {
    uint32_t branch;
    float score;
    double lwr;
} epik_amd_placement;

/*
 * What `epik::placer`'s constructor receives through `db` and `tree`
 * (place.cpp:83-96), flattened: the phylo-k-mer database as a CSR-like layout
 * (k-mer code -> posting list) replacing the i2l hash map behind
 * `phylo_kmer_db::search` (place.cpp:300,311).
 *
 * The code of a k-mer is the base-`alphabet_size` number of its k state codes, first
 * character most significant; num_keys must equal alphabet_size^kmer_size.  Two forms:
 *   dense  (keys == NULL): offsets[code] .. offsets[code+1] delimit the postings of `code` in
 *          values[]; offsets has num_keys + 1 entries -- 8 bytes per POSSIBLE k-mer, 10 GB for
 *          amino k = 7 whatever the database holds;
 *   sparse (keys != NULL, ABI 3): keys[num_present] are the codes that have a list, strictly
 *          ascending, and offsets[i] .. offsets[i+1] delimit the postings of keys[i]; offsets has
 *          num_present + 1 entries -- memory per PRESENT key, as the hash map behind
 *          phylo_kmer_db::search (place.cpp:300,311) has it.
 * All pointers are HOST pointers; create() streams them to the device (it keeps no copy and
 * needs no array of its own per code), the caller may free them afterwards.
 */
typedef struct {
    uint32_t abi_version;    /* EPIK_AMD_ABI_VERSION */
    uint32_t kmer_size;      /* db.kmer_size()                       place.cpp:87 */
    uint32_t alphabet_size;  /* 4 = nucl (epik-dna), 20 = amino (epik-aa); epik/CMakeLists.txt:72,124 */
    uint32_t num_branches;   /* tree.get_node_count()                place.cpp:92 */
    uint32_t keep_at_most;   /* --keep-at-most, default 7            main.cpp:219 */
    uint32_t offset_bits;    /* width of offsets[]: 32 or 64 */
    double keep_factor;      /* --keep-factor, default 0.01          main.cpp:220 */
    float threshold;         /* i2l::score_threshold(omega, k)       place.cpp:87 */
    float log_threshold;     /* std::log10(threshold), as float      place.cpp:88 */
    uint64_t num_keys;       /* alphabet_size ^ kmer_size */
    uint64_t num_entries;    /* the last offset = db.get_num_entries_loaded() */
    const void *offsets;     /* uint32_t/uint64_t [num_keys + 1] (dense) or [num_present + 1] (sparse) */
    const epik_amd_pkdb_value *values; /* [num_entries]; branches distinct within one list */
    const uint32_t *char_class; /* [256]: bit s set <=> the character may be state s;
                                   popcount 1 plain, >1 ambiguous, 0 invalid
                                   (i2l::to_kmers<one_ambiguity_policy>, place.cpp:294) */
    int32_t device;          /* HIP device ordinal */
    uint32_t shard;          /* 0: a whole database.  g | G << 16 (G >= 2, g < G): the descriptor holds shard g of G of one
                                ALREADY -- the lists of the codes with code % G == g and no others (k-mer-space shard,
                                below): create() then sizes its table for those codes alone, as create_sharded() does */
    const uint32_t *keys;    /* NULL: dense form; else [num_present] ascending codes (sparse form) */
    uint64_t num_present;    /* sparse form: number of codes that have a list */
} epik_amd_placer_desc;

typedef struct epik_amd_placer epik_amd_placer;

/* Number of visible HIP devices (0 when there is none / no driver). */
int epik_amd_device_count(void);

/* Message of the last failing call on this thread. */
const char *epik_amd_last_error(void);

/* Replaces epik::placer::placer (place.cpp:83-126): uploads the database to
 * the device's HBM once and precomputes what the kernel needs. */
int epik_amd_placer_create(const epik_amd_placer_desc *desc, epik_amd_placer **out);

/*
 * What create() would decide for this database on a device with `free_bytes` of free memory, and how
 * large the device image is -- without a device (capacity planning against 288 GB; no reference
 * counterpart: the reference keeps its hash map in host RAM, main.cpp:277).  `kernel` 0: one wavefront
 * places a read (trees whose score vector leaves enough waves on a CU); 1: the branch range is split into
 * team_waves * team_passes slices of `slice_rows` branches and a wavefront places one slice of a read
 * (large trees; place.cpp:92-96 bounds the tree by nothing, and neither does this).
 * The environment overrides of create() (EPIK_AMD_LAYOUT, EPIK_AMD_KERNEL) apply here too.
 */
typedef struct {
    uint32_t kernel;         /* 0 = one wavefront per read, 1 = one workgroup per read */
    uint32_t layout;         /* 0/1 compact CSR (32/64-bit offsets), 2 packed, 3 paired, 4 filtered, 5 sliced, 6 tripled */
    uint32_t team_waves;
    uint32_t team_passes;
    uint32_t slice_rows;
    uint32_t resident_waves[3]; /* one-wavefront kernel: waves per CU with 8/16/32-bit counts (0: does not fit) */
    uint64_t table_bytes;
    uint64_t filter_bytes;
    uint64_t posting_bytes;
    uint64_t kept_entries;   /* postings this placer keeps (its shard) */
    uint32_t run_coded;      /* 1: lists that are one ascending run of branches are stored without their cells
                                (4 bytes per posting; databases well beyond the Infinity Cache) */
    uint32_t posting_bytes_is_bound; /* epik_amd_placer_plan_sizes, sliced layout: posting_bytes is an upper bound */
} epik_amd_plan;
int epik_amd_placer_plan(const epik_amd_placer_desc *desc, uint32_t shard_index, uint32_t shard_count,
                         uint64_t free_bytes, epik_amd_plan *plan);
/*
 * The same plan from the SIZES of a database alone -- before it exists, or is at hand: the tree, the key space, and a
 * histogram of the posting lists the placer (shard shard_index of shard_count) will keep.  The reference's only
 * capacity control is --max-ram on the host (main.cpp:252-266, README.md:121-128); this answers "how many GPUs'
 * HBM does a database of this shape take, table included" without touching a posting.  kernel, layout, geometry,
 * resident_waves, table_bytes, filter_bytes, kept_entries and run_coded are what epik_amd_placer_plan() gives on
 * a database with these lists; posting_bytes too for the layouts of the one-wavefront kernel, and an upper bound
 * (a few percent: how a list falls over the slices of the branch range is not in a histogram) for the sliced
 * layout -- posting_bytes_is_bound says which.  No device needed.
 */
typedef struct {
    uint64_t length;         /* postings of a list */
    uint64_t lists;          /* lists of that length this placer keeps */
    uint64_t lists_in_runs;  /* ... of which are one ascending run of branches b, b + 1, ... (<= lists; 0 if unknown) */
} epik_amd_list_bin;
int epik_amd_placer_plan_sizes(uint32_t kmer_size, uint32_t alphabet_size, uint32_t num_branches, uint32_t keep_at_most,
                               const epik_amd_list_bin *bins, uint64_t n_bins, uint32_t shard_index, uint32_t shard_count,
                               uint64_t free_bytes, epik_amd_plan *plan);
/*
 * Whether the one-wavefront kernel keeps the k-mer counts per LIST, with counts of `counts` (0/1/2 = 8/16/32 bits):
 * *lists = 1 when the image is run-coded, every list the placer keeps is one ascending run of branches, and the counts
 * are 16 or 32 bits, in the packed and paired layouts -- each list then adds to its run's counts once, and the posting
 * ring carries scores only; 0: the counts go through the ring chunk by chunk (as for every other image).  The scores
 * and counts are the same either way.  EPIK_AMD_RUN_COUNTS (read at create()): `ring` keeps the chunk-by-chunk counts
 * everywhere, `lists` takes list counts in the filtered layout as well (by itself it keeps the ring there).  plan_run_counts: what
 * create() would choose for this database (no device); run_counts: what this handle does.
 */
int epik_amd_placer_plan_run_counts(const epik_amd_placer_desc *desc, uint32_t shard_index, uint32_t shard_count,
                                    uint64_t free_bytes, uint32_t counts, uint32_t *lists);
int epik_amd_placer_run_counts(const epik_amd_placer *p, uint32_t counts, uint32_t *lists);
/* How the posting ring of the one-wavefront kernel finds the chunks of a run-coded image, for that count width: 0 -- by
 * address or 128-byte line (any posting region; every image that is not run-coded); EPIK_AMD_RING_NEAR -- by 32-bit byte
 * offset under one buffer resource for the launch (posting regions shorter than 2^32 - 256 bytes; a stage of the
 * list-counts ring then takes 12 instructions instead of 19), there with EPIK_AMD_RING_SLACK where 64 slack rows behind
 * the wave's score vector cost no resident wave and replace the clamp of a lane's row.  The output is the same in every form.
 * EPIK_AMD_RING_FORM (read at create()): `far` keeps the line form; `near` is the default wherever it is legal. */
#define EPIK_AMD_RING_NEAR 1u
#define EPIK_AMD_RING_SLACK 2u
int epik_amd_placer_ring_form(const epik_amd_placer *p, uint32_t counts, uint32_t *form);
/* Which k-mer table the one-wavefront kernel of this handle looks its k-mers up in: keyed by code, by the (k-1)-mer two
 * consecutive k-mers of a read share (one 128-byte line per two lookups), or by the (k-1)-mer three of them share (one
 * line per three: 128 bytes per (k-1)-mer, 24 entries of 42 bits; 4-letter alphabets, k >= 3, whole databases whose kept
 * lists are all runs and take the near ring, entries that fit 42 bits).  The output is the same with every table.
 * EPIK_AMD_LAYOUT (read at create()): `tripled` asks for the last -- an error where the database cannot take it;
 * `paired` keeps the paired table.  By itself create() takes the tripled table where the paired one is larger than an
 * XCD's 4 MiB of L2 and the larger table does not move the image out of the 256 MiB Infinity Cache.
 * 0 for the sliced layout and the compact CSR. */
#define EPIK_AMD_TABLE_BY_CODE 1u
#define EPIK_AMD_TABLE_PAIRED 2u
#define EPIK_AMD_TABLE_TRIPLED 3u
int epik_amd_placer_table_form(const epik_amd_placer *p, uint32_t *form);
/* Where the one-wavefront kernel of this handle finishes a read, for that count width: EPIK_AMD_TAIL_WAVE -- in the wave
 * that placed it; EPIK_AMD_TAIL_KERNEL -- the wave stops behind the ranking of its candidates, and a second kernel,
 * enqueued behind the first on the same stream, computes 10^score, the LWRs and the filter with a lane per reported row
 * and writes rows, n_rows and k-mer counts (the kernels with list counts -- epik_amd_placer_run_counts -- of handles
 * with keep_at_most <= 64; placing launches only).  The output is the same bytes in either form, the slots past n_rows
 * included: nothing writes them.  EPIK_AMD_TAIL (read at create()): `wave` keeps the tail in the wave; `kernel` is the
 * default wherever that form exists. */
#define EPIK_AMD_TAIL_WAVE 0u
#define EPIK_AMD_TAIL_KERNEL 1u
int epik_amd_placer_tail_form(const epik_amd_placer *p, uint32_t counts, uint32_t *form);
/* The image create() uploads for that plan, written front to back into host buffers of
 * plan->table_bytes / filter_bytes / posting_bytes (NULL = that part is produced and dropped).
 * Host only; create() streams the same bytes to the device without holding them. */
int epik_amd_placer_build_image(const epik_amd_placer_desc *desc, uint32_t shard_index, uint32_t shard_count,
                                uint64_t free_bytes, void *table, void *filter, void *postings);

/* Replaces ~placer (place.h:100). */
void epik_amd_placer_destroy(epik_amd_placer *p);

/*
 * Replaces the OpenMP loop of epik::placer::place (place.cpp:218-268): places n
 * reads that the host has already de-duplicated (place.cpp:207-212).
 *   seqs / seq_offsets[n+1]: concatenated read bytes (HOST).
 *   rows[n * keep_at_most], n_rows[n]: placements in final order (sorted by
 *     score descending -- ties by branch ascending --, LWR-filtered,
 *     place.cpp:240-267); n_rows[i] == 0 iff read i is shorter than k.
 *   kmer_counts[n * keep_at_most] (nullable): placement::count (place.h:53).
 * Synchronous: copies in, runs the kernel, copies out.
 */
int epik_amd_placer_place(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets,
                          uint64_t n, epik_amd_placement *rows, uint32_t *n_rows,
                          uint32_t *kmer_counts);

/*
 * Same computation with every buffer already resident in device memory, enqueued
 * on `stream` (a hipStream_t passed as void*; NULL = the default stream) without
 * synchronising.  d_kmer_counts may be NULL.  The launches of one handle share its scratch
 * memory (large trees; the headers and candidates of EPIK_AMD_TAIL_KERNEL): enqueue them on one stream, or order them.
 * A call that has to allocate or grow that scratch (the first one, and one with more reads than any before it by more
 * than the head room) frees the old buffer first, which waits for the device; every other call only enqueues.
 * The call may enqueue more than one kernel: rows, n_rows and k-mer counts are final when `stream` reaches the end of
 * the last of them (with EPIK_AMD_TAIL_KERNEL, of the kernel that finishes the rows) -- for whoever reads them on the
 * same stream, behind an event recorded on it after the call, or after a synchronise.
 */
int epik_amd_placer_place_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets,
                                 uint64_t n, void *d_rows, void *d_n_rows, void *d_kmer_counts,
                                 void *stream);

/*
 * Measurement helper: algorithmic bytes of a device-resident
 * batch, sum over reads of L + 8*n_kmers + 8*sum|posting list| + 16*rows_out,
 * with rows_out taken from d_n_rows (NULL counts no output rows).  Synchronous.
 */
int epik_amd_placer_algorithmic_bytes(epik_amd_placer *p, const void *d_seqs,
                                      const void *d_seq_offsets, uint64_t n, const void *d_n_rows,
                                      void *stream, uint64_t *bytes_out);

/*
 * The kernel keeps one k-mer count per branch in LDS (the reference counts in size_t, place.h:86):
 * 16 bits by default (reads of up to 32767 k-mers), 32 bits for longer reads, 8 bits (reads of up to
 * 255 k-mers) when that lets more wavefronts share a CU -- large trees.  epik_amd_placer_place()
 * looks at the batch and chooses by itself; for the device-pointer entry points the caller chooses
 * here: enabled = 0 back to the default (16 bits, and place() chooses again), 1 = 32 bits, 2 = 8 bits
 * (EPIK_AMD_ERR_UNSUPPORTED for trees too large for that kernel).  A read with more k-mers than the
 * counts of a device-pointer launch hold is not placed and says so: n_rows == EPIK_AMD_ROWS_COUNTS_TOO_NARROW
 * (a read shorter than k has n_rows == 0).
 */
#define EPIK_AMD_ROWS_COUNTS_TOO_NARROW 0xffffffffu
int epik_amd_placer_set_wide_counts(epik_amd_placer *p, int enabled);
/* The same choice epik_amd_placer_place() makes, for the device-pointer entry points: the counts
 * that fit a batch whose longest read has `longest_read` characters. */
int epik_amd_placer_choose_counts(epik_amd_placer *p, uint64_t longest_read);

/*
 * Database larger than one GPU's memory: k-mer-space shard (BASELINE configs[4]).
 * No reference counterpart -- the reference keeps one database in host RAM (main.cpp:277).
 *
 * Shard g of G holds the posting lists of the k-mer codes with code % G == g.  Either hand create()
 * a descriptor that holds only those lists (every other code an empty list: no process then ever
 * holds the whole database -- create() streams what it is given to the device and keeps no copy), or
 * let epik_amd_placer_create_sharded() pick them out of a whole database
 * (create() == create_sharded(desc, 0, 1, out)).  Every shard then sees ALL reads of a batch:
 *
 *   accumulate_device : per read, the raw float32 score sums and the k-mer counts of this shard's
 *                       lists, d_scores float32 / d_counts uint16 = [n][num_branches]
 *                       (place.cpp:349-371 without 418-422); reads of up to 65535 k-mers (a longer one
 *                       leaves an all-zero vector and finish marks it EPIK_AMD_ROWS_COUNTS_TOO_NARROW:
 *                       the partial lists below have no such limit);
 *   (caller)          : adds d_scores and d_counts over the shards -- one all-to-all + a sum in rank
 *                       order, each GPU keeping the totals of its own reads (epik_amd/dist.py);
 *   finish_device     : correction, top-k, like-weight-ratio and filter on the totals
 *                       (place.cpp:418-422, 134-199, 241-267); rows as epik_amd_placer_place_device.
 *
 * Ambiguous k-mers (place.cpp:373-415): only the first ambiguous key that reaches a branch scores
 * it, first over the WHOLE database (:385-388).  A read that may hold an ambiguous character gets a
 * slot: d_amb_slot[i] >= 0 (int32, -1 = none) is its row in d_amb_order (uint32) and d_amb_avg
 * (float32), both [slots][num_branches].  accumulate fills that row, per branch, with the order
 * (k-mer position * alphabet_size + state) of the first ambiguous key of THIS shard that reached the
 * branch (0xffffffff: none) and its average probability (:400-402); the caller keeps, per branch, the
 * average of the smallest order over the shards (0 where there is none); finish adds it after the
 * exact scores and counts one k-mer, as the one-pass loop does (:409-410).  With d_amb_slot == NULL a
 * shard scores its ambiguous k-mers by itself -- the one-pass result with one shard only.
 *
 * With one shard the two calls give exactly the rows of place_device.  With several, a branch's
 * float32 adds happen in a different order (per shard, then over shards): scores agree to float32
 * rounding, like-weight-ratios within the 1e-5 bar.
 */
int epik_amd_placer_create_sharded(const epik_amd_placer_desc *desc, uint32_t shard_index,
                                   uint32_t shard_count, epik_amd_placer **out);
int epik_amd_placer_accumulate_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets,
                                      uint64_t n, void *d_scores, void *d_counts, const void *d_amb_slot,
                                      void *d_amb_order, void *d_amb_avg, void *stream);
int epik_amd_placer_finish_device(epik_amd_placer *p, const void *d_seq_offsets, uint64_t n,
                                  const void *d_scores, const void *d_counts, const void *d_amb_slot,
                                  const void *d_amb_avg, void *d_rows, void *d_n_rows, void *d_kmer_counts,
                                  void *stream);

/*
 * The same two halves with partial LISTS instead of dense vectors (large trees: the handles whose
 * epik_amd_placer_partial_info() says lists == 1).  A shard's lists reach a small part of a large tree per read
 * (N = 9 999, 8 shards: ~5 % of the branches), so accumulate leaves, per read and SLICE of the branch range
 * (slices * slice_rows >= num_branches; the same on every shard: the geometry depends on the tree alone), only the
 * rows that received a k-mer:
 *
 *   entry  {f32 sum, u32 row | count << 16}      8 bytes (counts of 8 or 16 bits: reads of up to 32767 k-mers)
 *          {f32 sum, u32 row, u32 count, u32 0}  16 bytes (32-bit counts, chosen for longer reads)
 *          row = branch - slice * slice_rows; any order inside a list, every row at most once;
 *   index  [n][slices] {u32 first, u32 count}: the list of (read, slice) = entries first .. first + count - 1 of
 *          the read's PART.
 *
 * The n reads form n_parts equal runs of ceil(n / n_parts) reads -- part r is what finisher r needs, and its
 * entries lie together: d_part_entries[r] (uint64) says how many entries part r takes in d_entries, the parts one
 * after the other from the start (lists are laid out before they are filled, from an upper bound -- the postings
 * of the slice's sublists --: a part is that bound added up, a few percent more than the entries its index names).
 * If the parts together exceed entries_cap the lists that found no room are marked count == 0xffffffff and the
 * call must be repeated with a larger buffer (read d_part_entries after the stream has finished; it is always
 * complete).  entries_cap < 2^32.
 *
 * finish_lists takes, for its n reads (one part), what each of the n_shards shards left for them: d_entries[g] =
 * the start of the part's entries as shard g wrote them, d_index[g] = the part's [n][slices] index of shard g
 * (HOST arrays of device pointers), and adds the lists of a slice into LDS in shard order -- the float32 sums
 * are those of the dense exchange's rank-order sum (0 + x is x) -- then finishes as finish_device does.  All
 * shards and the finisher must run with the same count width (epik_amd_placer_choose_counts with the batch's
 * longest read on each).  The ambiguous records cross as with the dense calls.
 * accumulate_lists and finish_lists of ONE handle may run side by side on two streams (the finish of a batch beside
 * the accumulate of the next: they keep separate scratch); two launches of the same kind may not.
 */
#define EPIK_AMD_MAX_SHARDS 16
typedef struct {
    uint32_t lists;        /* 1: accumulate_lists / finish_lists are available on this handle */
    uint32_t slices;       /* lists per read */
    uint32_t slice_rows;   /* branches per slice */
    uint32_t entry_bytes;  /* 8 or 16, for the count width chosen last */
    uint32_t num_branches;
    uint32_t reserved;
    double postings_per_kmer; /* mean postings of this shard's lists per k-mer code (to size d_entries:
                                 reads * k-mers per read * this, and some margin) */
} epik_amd_partial_info;
int epik_amd_placer_partial_info(const epik_amd_placer *p, epik_amd_partial_info *out);
int epik_amd_placer_accumulate_lists_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets,
                                            uint64_t n, uint32_t n_parts, void *d_entries, uint64_t entries_cap,
                                            void *d_index, void *d_part_entries, const void *d_amb_slot,
                                            void *d_amb_order, void *d_amb_avg, void *stream);
int epik_amd_placer_finish_lists_device(epik_amd_placer *p, const void *d_seq_offsets, uint64_t n, uint32_t n_shards,
                                        const void *const *d_entries, const void *const *d_index,
                                        const void *d_amb_slot, const void *d_amb_avg, void *d_rows, void *d_n_rows,
                                        void *d_kmer_counts, void *stream);

/*
 * The whole of it for a caller that drives all the devices from one process (epik-dna --db-shard): places n
 * HOST reads on `n_shards` handles that together hold one database -- handle g created with shard g of n_shards
 * (create() on a descriptor of its codes, or create_sharded()), on any devices, several on one if need be.
 * Replaces the OpenMP loop of epik::placer::place (place.cpp:218-268) as epik_amd_placer_place does, same
 * arguments and results.  Inside: chunks of the batch; every handle accumulates the partial lists of a chunk on
 * its device, part r of each goes to the device of handle r with one peer copy per pair (its own xGMI link),
 * handle r finishes its reads; the copies of a chunk run under the kernels of the next.  Reads with ambiguous
 * characters follow the first-key rule over all shards.  Large trees only (partial lists): a database that needs
 * several devices has one.  Synchronous; the handles must not be used by another thread meanwhile.
 */
int epik_amd_placer_place_sharded(epik_amd_placer *const *shards, uint32_t n_shards, const char *seqs,
                                  const uint64_t *seq_offsets, uint64_t n, epik_amd_placement *rows,
                                  uint32_t *n_rows, uint32_t *kmer_counts);

/*
 * Nucleotide reads placed on either strand.  No reference counterpart: the reference places a read in the
 * orientation it arrives in (place.cpp:294, to_kmers over the read as given).
 *   FORWARD  the read as given: the rows of place / place_device, strand 0 everywhere;
 *   REVERSE  its reverse complement, strand 1 everywhere;
 *   BOTH     both orientations, per read the better one: reverse when it has rows and either forward has none or
 *            its first score is strictly greater (float32) than forward's; else forward (a tie goes to forward).
 *            Rows, n_rows and k-mer counts are those of the chosen strand, LWRs not renormalised across strands.
 * The complement is taken on character classes: state s <-> 3 - s in the order A C G T, a 4-bit reversal of the
 * class bitmask (R <-> Y, K <-> M, B <-> V, D <-> H; S, W, N themselves; U -> A; invalid stays invalid).  The
 * reverse strand of read r has at position j the class bitrev4(char_class[r[len-1-j]]): its rows are those
 * place() gives for the host-side reverse complement of r.  strand[i]: 0 forward (+), 1 reverse (-).
 * Nucleotide handles of a whole database only: EPIK_AMD_ERR_UNSUPPORTED for alphabet_size != 4 or a k-mer-space
 * shard.  Deduplication stays the caller's, by exact string (place.cpp:73-81).
 *
 * place_strands_device: asynchronous on `stream`, count width as the caller chose it (as place_device); keeps no
 *   state of its own and never allocates: the caller provides d_workspace of at least the bytes
 *   strand_workspace_bytes gives for n reads and seq_bytes = d_seq_offsets[n] (the characters of the batch when
 *   its offsets start at 0): the reversed reads are written there at the caller's offsets.  FORWARD needs none.
 *   d_kmer_counts and d_strand (uint8 [n]) may be NULL.
 * place_strands: synchronous, host buffers; count width chosen from the batch's longest read as place() does,
 *   the handle's count state left as place() leaves it; the batch goes through the device in chunks of bounded
 *   size, allocated and freed inside the call.  kmer_counts and strand may be NULL.
 */
#define EPIK_AMD_STRAND_FORWARD 0u
#define EPIK_AMD_STRAND_REVERSE 1u
#define EPIK_AMD_STRAND_BOTH    2u
/* bytes of device workspace place_strands_device needs for n reads of seq_bytes characters in total */
int epik_amd_placer_strand_workspace_bytes(const epik_amd_placer *p, uint64_t n, uint64_t seq_bytes,
                                           uint32_t mode, uint64_t *bytes);
int epik_amd_placer_place_strands_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets,
                                         uint64_t n, uint32_t mode, void *d_workspace, uint64_t workspace_bytes,
                                         void *d_rows, void *d_n_rows, void *d_kmer_counts, void *d_strand,
                                         void *stream);
int epik_amd_placer_place_strands(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                  uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows,
                                  uint32_t *kmer_counts, uint8_t *strand);

/*
 * Paired-end reads placed jointly: one placement per fragment.  No reference counterpart: the reference knows single
 * reads only (place.cpp:294).
 *
 * The rule.  For a pair (m1, m2) of a nucleotide placer, with sep a byte of character class 0 (invalid) and rc() the
 * reverse complement on classes defined above:
 *     J = m1 . sep . rc(m2)     orientation FR (the default: Illumina paired-end)
 *     J = m1 . sep . m2         orientation FF (EPIK_AMD_MATES_FF)
 * The placement of the pair is the placement of J: rows, n_rows, k-mer counts and LWRs as epik_amd_placer_place gives
 * them for the string J.  Windows that contain sep are skipped as windows over any invalid character are, so every
 * branch receives the log-scores of both mates' k-mers, mate 1's first, in k-mer order.
 *   sep     '-' when its class in the handle's table is 0, else the smallest byte of class 0 (none:
 *           EPIK_AMD_ERR_UNSUPPORTED); mates_separator reports it, so that callers build the same J.
 *   Strand  rc(m1 . sep . rc(m2)) = m2 . sep . rc(m1): the reverse strand of J is the pair with its mates swapped.  The
 *           strand modes apply to J unchanged -- FORWARD: mate 1 lies on the database's strand; REVERSE; BOTH with the
 *           rule and tie-break of place_strands -- and strand[i] is 0 / 1 per pair.
 *   Consequences.  num_of_kmers is len(J) - k + 1 (place.cpp:322), which counts the k windows over sep as missing
 *           k-mers: every score of a pair is lower by exactly one log_threshold than the sum of its mates' evidence
 *           would give -- the same constant on every branch; ranking and LWRs do not depend on it.  A pair whose
 *           mates are both shorter than k while len(J) >= k comes back as a read without hits (fabricated rows, k-mer
 *           counts 0: no_hit in a profile), not with n_rows 0.  Mates that overlap count the shared k-mers twice.
 * The batch is ONE interleaved batch in the layout of reads: seqs + uint64 seq_offsets[2 n + 1], read 2 i = mate 1 and
 * read 2 i + 1 = mate 2 of pair i.  n counts pairs; rows [n][keep], n_rows [n], k-mer counts [n][keep] and strand [n]
 * are per pair.  mode = a strand mode (EPIK_AMD_STRAND_*) in the low byte, | EPIK_AMD_MATES_FF for FF; any other bit:
 * EPIK_AMD_ERR_INVALID.  Nucleotide handles of a whole database only (EPIK_AMD_ERR_UNSUPPORTED otherwise).
 *
 * place_mates_device: asynchronous on `stream`, never allocates.  seq_bytes = d_seq_offsets[2 n] - d_seq_offsets[0],
 *   the characters of the batch; d_workspace (aligned to 8 bytes) of at least mates_workspace_bytes(n, seq_bytes, mode)
 *   bytes, EPIK_AMD_ERR_INVALID when smaller: mate_join_kernel writes the joined sequences and their offsets
 *   (seq_offsets[2 i] - seq_offsets[0] + i) there, place_strands_device places them.  A pair whose offsets lie outside
 *   what seq_bytes says is not joined; nothing is written outside the workspace.  The count width is the caller's
 *   (epik_amd_placer_choose_counts with the longest J, len1 + len2 + 1: 2 x 150 bp needs 16-bit counts); a pair
 *   that does not fit comes back EPIK_AMD_ROWS_COUNTS_TOO_NARROW.  d_kmer_counts and d_strand may be NULL.  Row slots
 *   past n_rows[i] keep what the caller's buffers held -- in BOTH, where the reverse strand wins, what the workspace
 *   held: zero both beforehand to read zeros there, as place_mates does.
 * place_mates: synchronous, host buffers; count width chosen from the batch's longest J as place() does, the handle's
 *   count state left as place() leaves it; chunks of bounded size, by pairs, allocated and freed inside the call.
 *   kmer_counts and strand may be NULL.
 * profile_mates: place_mates with the rows left on the device and added to `profile` there (see below), pair i with
 *   weights[i] (HOST uint32 [n], or NULL: 1): a fragment counts once.
 */
#define EPIK_AMD_MATES_FF 0x100u
int epik_amd_placer_mates_separator(const epik_amd_placer *p, uint8_t *sep);
/* bytes of device workspace place_mates_device needs for n_pairs pairs of seq_bytes characters in total */
int epik_amd_placer_mates_workspace_bytes(const epik_amd_placer *p, uint64_t n_pairs, uint64_t seq_bytes,
                                          uint32_t mode, uint64_t *bytes);
int epik_amd_placer_place_mates_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets,
                                       uint64_t n_pairs, uint64_t seq_bytes, uint32_t mode, void *d_workspace,
                                       uint64_t workspace_bytes, void *d_rows, void *d_n_rows, void *d_kmer_counts,
                                       void *d_strand, void *stream);
int epik_amd_placer_place_mates(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n_pairs,
                                uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                uint8_t *strand);

/*
 * Nucleotide reads placed on an amino-acid database through their translated frames.  No reference counterpart: the
 * reference places a read in the alphabet of its database (place.cpp:294).
 *   FORWARD  frames +1 +2 +3;  REVERSE  frames -1 -2 -3;  BOTH  all six.
 * Frames.  Frame +f (f = 1, 2, 3) translates the codons that start at offset f-1 of the read; frame -f does the same
 *   on the reverse complement.  An incomplete trailing codon is dropped: a read of length L gives frames of
 *   floor((L - f + 1) / 3) residues (none when that is negative).  The reverse complement is the strand placement's:
 *   the class bitmask reversed, in A C G T order.
 * Codon -> residue: one 4096-entry byte table indexed by the three nucleotide class masks (4 bits each, the first
 *   nucleotide most significant), built in the library from the standard genetic code (NCBI table 1, which also
 *   serves table 11).  A codon with any class-0 (invalid) character becomes '*'.  Otherwise every combination of the
 *   codon's ambiguous characters (at most 64) is expanded: one amino acid -> that letter; only stops -> '*'; the
 *   amino-acid sets {D,N}, {E,Q} and {I,L} -> B, Z and J; any other set, a mix of stops and amino acids included,
 *   -> X.  U is T, and lower case is upper case.  '*' must be class 0 in the handle's class table (as in
 *   alphabet.py), so k-mers across a stop or a gap are skipped exactly as for invalid characters:
 *   EPIK_AMD_ERR_UNSUPPORTED otherwise.
 * Choosing a frame.  A frame has rows when its n_rows is neither 0 nor EPIK_AMD_ROWS_COUNTS_TOO_NARROW.  Its key is
 *   score[0] / (float)(len_f - k + 1), a float32 division rounded to nearest: the per-k-mer score (the raw score is
 *   not used: frames of one read differ by one residue, and the correction adds one log_threshold term per k-mer).
 *   The frame with rows and the strictly greatest key wins; ties go to the earlier frame in the order +1 +2 +3 -1 -2
 *   -3.  If no frame has rows, the read reports the first frame of the mode with that frame's n_rows (0).  If any
 *   frame of a read is TOO_NARROW, the read is TOO_NARROW.  Rows, counts and LWRs are the winning frame's and are not
 *   renormalised.  frame[i]: 0..5 for +1 +2 +3 -1 -2 -3.
 * Amino-acid handles of a whole database only: EPIK_AMD_ERR_UNSUPPORTED for alphabet_size != 20 or a k-mer-space
 * shard.  Deduplication stays the caller's, on the nucleotide string.
 *
 * place_frames_device: asynchronous on `stream`; never allocates: the caller provides d_workspace of at least the
 *   bytes frame_workspace_bytes gives for n reads and seq_bytes = d_seq_offsets[n] (the characters of the batch when
 *   its offsets start at 0).  All frames of the batch are placed in ONE call of epik_amd_placer_place_device, with
 *   the count width the caller chose (epik_amd_placer_choose_counts with the longest FRAME, floor(L / 3)).
 *   d_kmer_counts and d_frame (uint8 [n]) may be NULL.
 * place_frames: synchronous, host buffers; count width chosen from the batch's longest frame, the handle's count
 *   state left as place() leaves it; the batch goes through the device in chunks of bounded size, allocated and
 *   freed inside the call.  kmer_counts and frame may be NULL.
 * codon_table: the 4096-entry table above (needs no device).
 */
#define EPIK_AMD_FRAMES_FORWARD 0u
#define EPIK_AMD_FRAMES_REVERSE 1u
#define EPIK_AMD_FRAMES_BOTH    2u
int epik_amd_codon_table(uint8_t *out);  /* out: 4096 bytes */
/* bytes of device workspace place_frames_device needs for n reads of seq_bytes characters in total */
int epik_amd_placer_frame_workspace_bytes(const epik_amd_placer *p, uint64_t n, uint64_t seq_bytes,
                                          uint32_t mode, uint64_t *bytes);
int epik_amd_placer_place_frames_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets,
                                        uint64_t n, uint32_t mode, void *d_workspace, uint64_t workspace_bytes,
                                        void *d_rows, void *d_n_rows, void *d_kmer_counts, void *d_frame,
                                        void *stream);
int epik_amd_placer_place_frames(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                 uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows,
                                 uint32_t *kmer_counts, uint8_t *frame);

/*
 * The abundance profile of a sample, summed on the device from the rows a placement wrote.  No reference counterpart:
 * the reference writes every read into a jplace (main.cpp:355-361) and leaves the sums to a second tool.
 *
 * Per branch, mass = the summed like-weight ratios of the rows on it, in fixed point, and best = the reads whose first
 * row is on it; per sample, how many reads were placed, had no hit, were too short.  One rule:
 *   q(x) = llrint(x * 2^EPIK_AMD_PROFILE_LWR_BITS), round half to even, for a double x in [0, 1].
 *   Read i with weight w (uint32; 1 without weights; 0 adds nothing), keep = keep_at_most, tested in this order:
 *     n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW   totals.too_narrow += w
 *     n_rows[i] == 0                                 totals.too_short  += w
 *     kmer_counts[i * keep] == 0                     totals.no_hit     += w
 *     otherwise                                      totals.placed     += w;  best[rows[i * keep].branch] += w;
 *                                                    mass[rows[i * keep + j].branch] += w * q(rows[i * keep + j].lwr), j < n_rows[i]
 *   The third line is the read none of whose k-mers is in the database: place.cpp:141-152 gives it keep_at_most
 *   fabricated rows on branches 0, 1, 2, ... with LWR 1 / num_branches each, which a jplace cannot tell from
 *   placements; their k-mer counts are 0.  A row of a placed read whose branch is >= num_branches (never from this
 *   library) writes nothing and adds 1 to totals.bad_rows.  LWRs are taken as reported (after the keep_factor filter,
 *   not renormalised).  Every accumulator is a uint64 and wraps modulo 2^64 (2^34 weighted reads on one branch).
 * Integer adds commute: the result is the same bits whatever the batch size, the chunks, the grid, the number of
 * profiles summed afterwards or the order of the calls.
 *
 * An epik_amd_profile is an object of its own, created for a placer's device, num_branches and keep_at_most (the
 * placer may be destroyed before it); all zero at create() and after reset().
 *   add_device  asynchronous on `stream` (a hipStream_t as void*; NULL = the default stream), allocates nothing: adds
 *               the n reads whose rows [n][keep], n_rows [n] and k-mer counts [n][keep] a placement left in device
 *               memory -- d_kmer_counts is required --, read i with d_weights[i] (uint32 [n]; NULL: 1).  n == 0 does
 *               nothing.  Adds of one profile may run on several streams at once.
 *   read        synchronises the profile's device, then copies out mass[num_branches], best[num_branches] and the
 *               totals (each may be NULL).
 *   reset       synchronises the device and zeroes the profile.
 *   info        num_branches, and whether add_device sums in LDS first (trees whose 16 * num_branches bytes fit: up to 10 236) or
 *               straight into global memory; EPIK_AMD_PROFILE_LDS=0|1, read at create(), forces either (tests).
 * profile_reads / _strands / _frames / _mates: place / place_strands / place_frames / place_mates with the rows left on
 * the device and added to `profile` there -- nothing crosses back but the strand / frame byte per read or pair (NULL:
 * nothing at all).  weights: uint32 [n] on the HOST, or NULL; profile_mates: n pairs, a weight per pair.  The profile must have been created for this placer's device and shape.  Whole
 * databases only.  Synchronous.
 */
#define EPIK_AMD_PROFILE_LWR_BITS 30
typedef struct epik_amd_profile epik_amd_profile;
typedef struct {
    uint64_t placed;     /* weighted reads with rows and hits */
    uint64_t no_hit;     /* ... whose rows are fabricated: none of their k-mers is in the database */
    uint64_t too_short;  /* ... shorter than k */
    uint64_t too_narrow; /* ... EPIK_AMD_ROWS_COUNTS_TOO_NARROW (device-pointer launches only) */
    uint64_t bad_rows;   /* rows (not weighted) whose branch is >= num_branches */
} epik_amd_profile_totals;
int epik_amd_profile_create(const epik_amd_placer *p, epik_amd_profile **out);
void epik_amd_profile_destroy(epik_amd_profile *profile);
int epik_amd_profile_reset(epik_amd_profile *profile);
int epik_amd_profile_read(epik_amd_profile *profile, uint64_t *mass, uint64_t *best, epik_amd_profile_totals *totals);
int epik_amd_profile_info(const epik_amd_profile *profile, uint32_t *num_branches, uint32_t *lds_path);
int epik_amd_profile_add_device(epik_amd_profile *profile, const void *d_rows, const void *d_n_rows,
                                const void *d_kmer_counts, const void *d_weights, uint64_t n, void *stream);
int epik_amd_placer_profile_reads(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs,
                                  const uint64_t *seq_offsets, const uint32_t *weights, uint64_t n);
int epik_amd_placer_profile_strands(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs,
                                    const uint64_t *seq_offsets, const uint32_t *weights, uint64_t n, uint32_t mode,
                                    uint8_t *strand);
int epik_amd_placer_profile_frames(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs,
                                   const uint64_t *seq_offsets, const uint32_t *weights, uint64_t n, uint32_t mode,
                                   uint8_t *frame);
int epik_amd_placer_profile_mates(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs,
                                  const uint64_t *seq_offsets, const uint32_t *weights, uint64_t n_pairs, uint32_t mode,
                                  uint8_t *strand);

/*
 * Per-read placement confidence, computed on the device from the rows a placement wrote: the LCA clade that holds a
 * given share of the read's placement mass, and the EDPL (expected distance between placement locations).  No reference
 * counterpart: the reference writes a jplace and leaves both to a second tool.  One rule; the kernel
 * (confidence_place.hip), the host mirror (epik_amd/host/confidence.cpp) and the tests' numpy are worded after it and
 * must agree bit for bit, edpl included.
 *
 * The tree.  N = num_branches nodes with post-order ids; branch b joins node b to parent[b]; parent[b] > b for
 *   b < N - 1 and parent[N - 1] = EPIK_AMD_TREE_NO_PARENT.  size[b] = the nodes of the subtree of b, b included;
 *   first[b] = b - size[b] + 1; x lies in the clade of b <=> first[b] <= x <= b.  create() / build_host() refuse with
 *   EPIK_AMD_ERR_INVALID and a message that names the branch ("branch <b>: ..."), checked in ascending b, per branch in
 *   this order: a branch length that is negative or not finite; a second root (b < N - 1 without parent); a root with a
 *   parent (b = N - 1); a parent not above its child (parent[b] <= b, or >= N); a node whose descendants are not
 *   exactly [first[b], b].  Multifurcating trees and N = 1 are valid.
 *   depth[b] = depth[parent[b]] + branch_length[b], the root's parent counting as depth 0: one double add each, from
 *   the root down.  mid[b] = depth[b] - branch_length[b] / 2: a placement sits at the middle of its branch
 *   (distal_length = branch_length / 2, place.cpp:110, 435); pendant lengths take no part.
 *   lca(a, b) = the ancestor-or-self c of max(a, b), lowest in the tree, with first[c] <= min(first[a], first[b]).
 *   d(a, a) = 0; if a lies in the clade of b, d(a, b) = mid[a] - mid[b], and the other way round; otherwise, with
 *   c = lca(a, b), d(a, b) = (mid[a] - depth[c]) + (mid[b] - depth[c]), evaluated as parenthesised.
 *
 * The record of read i.  q() is the profile's; keep = keep_at_most; nr = min(n_rows[i], keep).  Tested in this order:
 *     n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW    clade = EPIK_AMD_CLADE_TOO_NARROW, the other fields 0
 *     n_rows[i] == 0                                  clade = EPIK_AMD_CLADE_TOO_SHORT,  the other fields 0
 *     kmer_counts[i * keep] == 0                      clade = EPIK_AMD_CLADE_NO_HIT,     the other fields 0
 *     a row j < nr with branch >= N                   clade = EPIK_AMD_CLADE_BAD_ROW,    the other fields 0
 *   (the third: the rows fabricated for a read without hits, place.cpp:141-152, produce no clade).  Otherwise, with
 *   b_j and lwr_j the branch and like-weight ratio of row j:
 *   clade         S_m = sum over j < m of q(lwr_j), S = S_nr; m = the smallest m >= 1 with S_m * 2^30 >= tau_q * S in
 *                 uint64 (nr when there is none: only sums that wrap); tau_q in [0, 2^30], larger is
 *                 EPIK_AMD_ERR_INVALID.  Rows come in (score descending, branch ascending) order: the prefix is the
 *                 best rows.  clade = the lca of b_0 ... b_(m-1), folded left to right; tau_q = 0 gives b_0,
 *                 tau_q = 2^30 the lca of all rows.
 *   clade_mass_q  the sum of q(lwr_j) over all j < nr with first[clade] <= b_j <= clade, saturating at 2^32 - 1.
 *   edpl          2 * sum over j < l < nr of (lwr_j * lwr_l) * d(b_j, b_l): the products as parenthesised, the pairs
 *                 added in lexicographic (j, l) order, in double, round to nearest, multiply and add never fused; the
 *                 sum over ordered pairs with the LWRs as reported (after keep_factor, not renormalised), as the
 *                 profile takes them.  nr = 1 gives +0.0.
 *   The rule reads slots past n_rows nowhere.  The record is a pure function of the read's rows and the tree: the same
 *   bits whatever the grid, the chunks or the stream.
 *
 * An epik_amd_tree is an object of its own on `device`, independent of any placer.  It holds first, depth, mid and,
 * for lca, binary lifting over parent[]: lift[l][b] = {the 2^l-th ancestor u of b (the root where there is none),
 * first[u]}, l < levels = max(1, ceil(log2 N)) -- a query is at most levels + 1 dependent loads on any valid tree.
 *   tree_create      validates, builds the tables on the host and uploads them.  EPIK_AMD_MAX_BLOCKS, read here, caps
 *                    the grid of confidence_device (tests).
 *   tree_info        num_branches, levels and the bytes of the tables (each may be NULL).
 *   tree_build_host  the same tables into host memory, without a device: *table_bytes = their size; tables == NULL
 *                    asks for the size alone.  tree_lca_host answers n queries on such tables with the very function
 *                    the kernel calls (a[i], b[i] < N, else EPIK_AMD_ERR_INVALID).
 *   confidence_device  asynchronous on `stream`, allocates nothing: d_out[i] for the n reads whose rows [n][keep],
 *                    n_rows [n] and k-mer counts [n][keep] (required) a placement left in device memory; n == 0 does
 *                    nothing.  keep in [1, 64], as a placer's keep_at_most.
 *   confidence_reads / _strands / _frames / _mates: place / place_strands / place_frames / place_mates with `conf`
 *                    [n] records (HOST) computed on the device from each chunk's rows; rows, n_rows and kmer_counts
 *                    may be NULL, each by itself: that part stays on the device.  `profile` (optional): the rows are
 *                    also added to it there, item i with weights[i] (HOST uint32 [n], or NULL: 1; without a profile
 *                    the weights are not looked at).  The tree must be on the placer's device and have its
 *                    num_branches.  Whole databases only.  Synchronous.
 */
#define EPIK_AMD_TREE_NO_PARENT 0xffffffffu
#define EPIK_AMD_CLADE_TOO_NARROW 0xffffffffu
#define EPIK_AMD_CLADE_TOO_SHORT 0xfffffffeu
#define EPIK_AMD_CLADE_NO_HIT 0xfffffffdu
#define EPIK_AMD_CLADE_BAD_ROW 0xfffffffcu
typedef struct {
    uint32_t clade;
    uint32_t clade_mass_q;
    double edpl;
} epik_amd_confidence; /* 16 bytes */
typedef struct epik_amd_tree epik_amd_tree;
int epik_amd_tree_create(int32_t device, const uint32_t *parent, const double *branch_length, uint32_t num_branches,
                         epik_amd_tree **out);
void epik_amd_tree_destroy(epik_amd_tree *tree);
int epik_amd_tree_info(const epik_amd_tree *tree, uint32_t *num_branches, uint32_t *levels, uint64_t *table_bytes);
int epik_amd_tree_build_host(const uint32_t *parent, const double *branch_length, uint32_t num_branches, void *tables,
                             uint64_t *table_bytes);
int epik_amd_tree_lca_host(const void *tables, const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t *out);
int epik_amd_confidence_device(const epik_amd_tree *tree, const void *d_rows, const void *d_n_rows,
                               const void *d_kmer_counts, uint64_t n, uint32_t keep, uint32_t tau_q, void *d_out,
                               void *stream);
int epik_amd_placer_confidence_reads(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                     epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                     const epik_amd_tree *tree, uint32_t tau_q, epik_amd_confidence *conf,
                                     epik_amd_profile *profile, const uint32_t *weights);
int epik_amd_placer_confidence_strands(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                       uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                       uint8_t *strand, const epik_amd_tree *tree, uint32_t tau_q,
                                       epik_amd_confidence *conf, epik_amd_profile *profile, const uint32_t *weights);
int epik_amd_placer_confidence_frames(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                      uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                      uint8_t *frame, const epik_amd_tree *tree, uint32_t tau_q,
                                      epik_amd_confidence *conf, epik_amd_profile *profile, const uint32_t *weights);
int epik_amd_placer_confidence_mates(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n_pairs,
                                     uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                     uint8_t *strand, const epik_amd_tree *tree, uint32_t tau_q,
                                     epik_amd_confidence *conf, epik_amd_profile *profile, const uint32_t *weights);

/*
 * A cohort: the profiles of many samples placed on one tree, summed on the device, and the phylogenetic
 * Kantorovich-Rubinstein (earth mover's) distance between every two of them.  No reference counterpart.  One rule
 * (DESIGN.md 3.8); the kernels (cohort_place.hip), the host mirror (epik_amd/host/cohort.cpp) and the tests' numpy are
 * worded after it and must agree bit for bit, the distances included.
 *
 * Cohort cells.  A cohort of S = num_samples samples over N = num_branches branches is S rows of
 *   mass[N] | best[N] | totals[5], every cell a uint64 that wraps, laid out as a profile is.  Read i belongs to sample
 *   samples[i] (uint32).  samples[i] < S: the read is added to that row by exactly the profile's rule above -- the four
 *   classes in its order, q(lwr) = llrint(lwr * 2^30), the weights, bad_rows.  samples[i] >= S: the read adds to no row
 *   and adds 1 (not its weight) to the cohort-wide counter bad_samples; nothing is written out of range.
 *   Integer adds commute: the cells are the same bits whatever the order of the reads, the grouping of the samples, the
 *   pieces, the grid, the stream or the number of devices whose cohorts are summed afterwards (add_cells).
 *
 * KR distance.  From mass[s][b], the tree's first[b] (the clade of b is the post-order id range [first[b], b]) and
 *   branch_length[b], finite and >= 0.  Per sample s, in uint64 (wrapping; exact below 2^64):
 *     T_s        = sum over b of mass[s][b]
 *     clade_s[b] = sum over x = first[b] .. b of mass[s][x]        (a difference of the prefix sum)
 *     below_s[b] = clade_s[b] - mass[s][b]
 *     C_s[b] = (double)clade_s[b] / (double)T_s,  B_s[b] = (double)below_s[b] / (double)T_s
 *   each one uint64 -> double conversion, round to nearest even, and one correctly rounded division.  A placement sits
 *   at the middle of its branch (place.cpp:110, 435): below a point of the distal half of b lies below_s[b] of the mass,
 *   of the proximal half clade_s[b].  Pendant lengths take no part.
 *     KR(s, t) = acc after, for b = 0, 1, ..., N - 1 in THIS order, in double, nothing fused:
 *                acc = acc + (0.5 * bl[b]) * (|C_s[b] - C_t[b]| + |B_s[b] - B_t[b]|),     acc = +0.0 at first
 *   KR(s, s) = +0.0.  T_s == 0 or T_t == 0 and s != t: -1.0, no distance.  |x - y| = |y - x| bit for bit, so the matrix
 *   is symmetric.  The sum over b is strictly sequential per pair: an implementation may share out the pairs, never
 *   the branches of one pair.
 *
 * UniFrac distances: unweighted (Lozupone & Knight 2005), normalised weighted (Lozupone et al. 2007) and
 *   generalised at alpha = 0.5 (Chen et al. 2012).  From C_s[b], B_s[b], T_s, first[] and h_b = 0.5 * bl[b] exactly as the KR
 *   rule has them: a placement sits at the middle of its branch, so a branch is two half-branches with the shares C
 *   (proximal half) and B (distal half).  The tree is taken as rooted where the database's tree is (post-order, the root
 *   last): KR does not depend on the rooting, UniFrac does.  For a pair (s, t), num = den = +0.0 at first, then for
 *   b = 0, 1, ..., N - 1 in THIS order, in double, nothing fused:
 *       num = num + h_b * tn_b,        den = den + h_b * td_b
 *   with, by metric (the id is EPIK_AMD_DISTANCE_*; [p] is 1 where p holds, else 0):
 *     unweighted (1)   tn_b = (double)([C_s>0] != [C_t>0]) + (double)([B_s>0] != [B_t>0])
 *                      td_b = (double)([C_s>0] or [C_t>0]) + (double)([B_s>0] or [B_t>0])
 *     weighted (2)     tn_b = |C_s - C_t| + |B_s - B_t|   (KR's term),       td_b = (C_s + C_t) + (B_s + B_t)
 *     generalized (3)  tn_b = g(C_s, C_t) + g(B_s, B_t),  g(x, y) = (x + y) > 0 ? sqrt(x + y) * (|x - y| / (x + y)) : 0
 *                      td_b = sqrt(C_s + C_t) + sqrt(B_s + B_t)
 *   sqrt and every division correctly rounded.  Then, in this order: D(s, s) = +0.0; D(s, t) = -1.0 where T_s == 0 or
 *   T_t == 0, as KR writes it; D(s, t) = +0.0 where den == 0; otherwise D(s, t) = num / den, one correctly rounded
 *   division.  So weighted's num is KR(s, t) bit for bit, all three lie in [0, 1], two samples with disjoint support are
 *   at unweighted 1.0 and identical rows at 0.0, exactly.  The sum over b is strictly sequential per pair, as KR's.
 *   Other alpha (they need pow), variance-adjusted UniFrac and UniFrac for squash and k-means are left out.
 *
 * Squash clustering (Matsen & Evans 2013) of the cohort's samples.  From mass[S][N], first[N] and branch_length[N] as
 *   for the KR distance; T_s, C_s[b], B_s[b] are exactly those above, and KR(x, y) over ANY two pairs of planes
 *   (C_x, B_x), (C_y, B_y) is the sequential sum above: acc = +0.0, then for b = 0 .. N - 1 in this order, in double,
 *   nothing fused, acc = acc + (0.5 * bl[b]) * (|C_x[b] - C_y[b]| + |B_x[b] - B_y[b]|).
 *   Slots.  Slot s = sample s, s in [0, S).  A slot is live iff T_s > 0: empty samples are never clustered.
 *     w[s] = 1, node[s] = s, D[r][c] = KR(r, c) for live r != c (the matrix epik_amd_cohort_kr gives).
 *   Step t = 0, 1, ...: scan the pairs (r, c), r < c, both live, in row-major order (r ascending, then c ascending) and
 *     take the FIRST pair with the smallest D[r][c] (strict <: ties go to the earlier pair).  With fewer than two live
 *     slots the clustering is over.
 *   Merged planes, for every b, W = (double)(w[r] + w[c]), each operation rounded on its own:
 *     C_m[b] = ((double)w[r] * C_r[b] + (double)w[c] * C_c[b]) / W,        B_m[b] likewise.
 *   Record t = {a = node[r], b = node[c], dist = D[r][c], len_a = KR(m, r), len_b = KR(m, c)}, the two lengths with
 *     the planes of r and c as they were before the merge.
 *   Then slot r takes the planes of m, w[r] += w[c], node[r] = S + t, slot c dies, and D[r][x] = D[x][r] = KR(m, x)
 *     for every live x != r.
 *   Result.  max(0, live - 1) merges; the records past them are {0xffffffff, 0xffffffff, 0, 0, 0}.  The sum over b
 *     stays strictly sequential per pair: an implementation may share out the clusters x, the branches of the
 *     AVERAGING and the scan, never the branches of one distance.
 *
 * Edge principal components (Matsen & Evans 2013) of the cohort's samples.  From mass[S][N], first[N] and K in [1, 64];
 *   no branch lengths.  All arithmetic is IEEE double, every operation rounded on its own, nothing fused.
 *   Used samples.  T_s, C_s[b], B_s[b] are exactly those of the KR rule.  Sample s is used iff T_s > 0; the used
 *     samples, in ascending s, get the indices j = 0 .. L - 1.  L may be 0.
 *   Imbalance.  Branch b is inner iff first[b] < b.  For an inner b, X_j[b] = (B_s[b] + C_s[b]) - 1.0: the mass strictly
 *     distal of b minus the mass strictly proximal of it, the branch's own mass on neither side (as guppy and gappa
 *     count it).  For every other b, X_j[b] = +0.0.
 *   Centring.  mean[b] = (acc after j = 0 .. L - 1 in this order, acc = acc + X_j[b], acc = +0.0 at first) / (double)L,
 *     Y_j[b] = X_j[b] - mean[b].
 *   Gram matrix.  For i <= j, G[i][j] = acc after b = 0 .. N - 1 in THIS order, acc = acc + (Y_i[b] * Y_j[b]),
 *     acc = +0.0 at first; G[j][i] = G[i][j].  The sum over b is strictly sequential per pair: an implementation may
 *     share out the pairs, never the branches of one pair.  scale = max over j of G[j][j] (+0.0 for L = 0); trace = the
 *     sequential sum of G[j][j], j ascending, from +0.0; tol = 2^-52 * scale.
 *   Eigen-decomposition: cyclic Jacobi in round-robin order, the rotations of a round applied together.  A = G, V = I,
 *     m = L + (L mod 2).  A sweep is the rounds r = 0 .. m - 2; round r holds the pairs {r, m - 1} and, for
 *     i = 1 .. m/2 - 1, {(r + i) mod (m - 1), (r - i + m - 1) mod (m - 1)}, each ordered (p, q) with p < q.  A pair with
 *     q >= L (the phantom index of an odd L) does nothing.  For every other pair, from A as it is at the START of the
 *     round: apq = A[p][q]; the pair rotates iff |apq| > tol, and then
 *       theta = (A[q][q] - A[p][p]) / (2.0 * apq),   t = 1.0 / (|theta| + sqrt(theta * theta + 1.0)), negated iff theta < 0,
 *       c = 1.0 / sqrt(t * t + 1.0),   s = t * c;
 *     index p gets (c_p, s_p, p') = (c, s, q), index q gets (c_q, s_q, q') = (c, -s, p).  Then three phases, in order:
 *       column phase, on the full matrix: for every i and every rotating j, A1[i][j] = c_j * A[i][j] - s_j * A[i][j'],
 *         two products then one subtraction; other elements are unchanged.  V1[i][j] likewise from V.
 *       row phase: for i <= j with i rotating, A2[i][j] = c_i * A1[i][j] - s_i * A1[i'][j]; otherwise
 *         A2[i][j] = A1[i][j].  Then A2[j][i] = A2[i][j].
 *       for every rotated pair A2[p][q] = A2[q][p] = +0.0.
 *     Sweeps run until a whole sweep rotates no pair: converged = 1, and `sweeps` counts that last sweep too.  After 64
 *     sweeps at the latest: converged = 0, and the results are taken from A and V as they stand.  L <= 1: one empty sweep.
 *   Components.  mu_j = A[j][j], ordered by (mu descending, j ascending); K' = min(K, L); component k is null iff
 *     !(mu_k > 2^-40 * scale).  For a non-null k, with j(k) the column of V it came from: r = sqrt(mu_k);
 *     raw[b] = the sum over j = 0 .. L - 1 in this order of V[j][j(k)] * Y_j[b], from +0.0; b* = the first b with the
 *     largest |raw[b]|, sign = -1 iff raw[b*] < 0, else +1;
 *       edge[k][b] = sign * (raw[b] / r),      proj[s][k] = sign * (V[j(s)][j(k)] * r).
 *     Both are +0.0 for a null k, for k >= K' and for an unused s.  mu[k] is written as computed for k < K', +0.0 beyond.
 *   The files derive, one division each: lambda_k = mu_k / (double)max(L - 1, 1); fraction_k = mu_k / trace, 0 when
 *     trace is 0.
 *
 * Phylogenetic k-means (Czech et al. 2019) of the cohort's samples.  From mass[S][N], first[N], branch_length[N] as for
 *   the KR distance, K in [1, 64] and max_iterations in [1, 1000].  All arithmetic is IEEE double, every operation
 *   rounded on its own, nothing fused.  T_s, C_s[b], B_s[b] are exactly those of the KR rule, and KR(x, y) over ANY two
 *   pairs of planes is the KR rule's sequential sum: acc = +0.0, then for b = 0 .. N - 1 in this order
 *   acc = acc + (0.5 * bl[b]) * (|C_x[b] - C_y[b]| + |B_x[b] - B_y[b]|).  An implementation may share out the (sample,
 *   centroid) pairs and the branches of an AVERAGING, never the branches of one distance or the members of one average.
 *   Used samples.  Sample s is used iff T_s > 0; the used samples, in ascending s, get j = 0 .. L - 1.  K' = min(K, L).
 *     L = 0: info = {0, 0, 0, 1} and every other output as for an unused sample or a cluster >= K'.
 *   Seeding (farthest first, deterministic).  Grand mean: M.C[b] = (acc after j = 0 .. L - 1 in this order,
 *     acc = acc + C_j[b], acc = +0.0 at first) / (double)L, M.B likewise.  Centre 0 is the first j with the smallest
 *     KR(M, j) (strict <); then mind[j] = KR(centre 0, j).  Centre k = 1 .. K' - 1 is the first j, not yet a centre, with
 *     the largest mind[j] (strict >; a mind of 0 qualifies, so two identical samples can both become centres); then
 *     mind[j] = min(mind[j], KR(centre k, j)).  Centroid k starts as the planes of centre k; seed[k] is that centre's
 *     sample index s (not j).
 *   Iteration i = 1, 2, ..., in this order:
 *     1. D[j][k] = KR(j, centroid k) for all j and k < K'.
 *     2. new[j] = the first k with the smallest D[j][k] (strict <).  changed = the number of j with new[j] != assign[j];
 *        assign is "none" before iteration 1, so iteration 1 never converges when L >= 1.  Then assign = new.
 *     3. changed == 0: converged = 1, iterations = i, stop.
 *     4. i == max_iterations: converged = 0, iterations = i, stop (no update follows the last assignment).
 *     5. Update, for every k with at least one member: centroid_k.C[b] = (acc after its members in ascending j,
 *        acc = acc + C_j[b], acc = +0.0 at first) / (double)size_k, .B likewise.  A cluster without members keeps the
 *        planes it has.
 *   Results.  Per sample {cluster, 0, dist}, dist = D[j][assign[j]] of the last step 1; an unused sample gets
 *     {0xffffffff, 0, -1.0}.  Per cluster k < K {size, seed, sum_dist, sum_sq}, the two sums over the members in
 *     ascending j from +0.0, sum_sq adding dist * dist; {0, 0xffffffff, +0.0, +0.0} for k >= K'.
 *     centroids[K][N] = centroid_k.C[b] - centroid_k.B[b], the centroid's own mass on b, +0.0 for k >= K'.
 *     info = {used L, clusters K', iterations, converged}.  Every cell of every output is written.
 *
 * Alpha diversity and rarefaction (McCoy & Matsen 2013; Nipperess & Matsen 2013) of the cohort's samples: how diverse
 *   each sample is, and whether it was sequenced deeply enough to say.  From mass[S][N] (the indices), best[S][N] (the
 *   curve), first[N] and branch_length[N] as for the KR distance.  All arithmetic is IEEE double, every operation rounded
 *   on its own, nothing fused; + - * /, sqrt (correctly rounded), min and comparisons only.  Denormals take part as IEEE
 *   says.  Phylogenetic entropy (-D log D) and BWPD at a general theta are deliberately left out: no log or pow gives
 *   the same bits in the kernels, on the host and in numpy.
 *   Blocked sum BS(t) over the branches, EPIK_AMD_DIVERSITY_BLOCK = 256: block g covers b = 256 g .. min(256 g + 255,
 *     N - 1); p_g = acc after those b in ascending order, acc = acc + t[b], acc = +0.0 at first; BS = acc after g
 *     ascending, acc = acc + p_g, from +0.0.  A fixed order, as the sequential one is; blocked because here the branches,
 *     not the pairs, are the parallelism (64 samples must still fill the device).  An implementation may share out the
 *     samples, the blocks and the depths, never the branches of one block or the blocks of one sum.
 *   half[b] = 0.5 * bl[b].  A placement sits at the middle of its branch, so a branch is two half branches: the distal
 *     one with `below` on its far side, the proximal one with `clade`.
 *   Alpha indices, from mass.  T_s, clade_s[b], below_s[b], C_s[b], B_s[b] are exactly those of the KR rule.  For a half
 *     branch with the integer x (below or clade) and D (B or C):
 *       u(x) = 1.0 iff 0 < x < T_s (integer compare), else +0.0        r(x) = 1.0 iff x > 0, else +0.0
 *       w(D) = min(D, 1.0 - D), replaced by +0.0 unless w > 0.0
 *       h(D) = sqrt(2.0 * w)        l(D) = 2.0 * w        e(D) = D * (1.0 - D)
 *     For each f of the five, term_f[b] = half[b] * (f(distal) + f(proximal)), and
 *       alpha[s] = {pd = BS(term_u), rooted_pd = BS(term_r), bwpd_half = BS(term_h), bwpd_one = BS(term_l),
 *                   quadratic = BS(term_e)};      T_s == 0: all five are -1.0.
 *     With cells that wrapped the values mean nothing, but they are still these bits.
 *   Rarefaction, from best (every read a unit mass at its best branch, as guppy rarefact takes it).  In uint64, wrapping:
 *       n_s = sum over b of best[s][b],   cc_s[b] = sum over x = first[b] .. b of best[s][x],   cb_s[b] = cc_s[b] - best[s][b].
 *     A sample is rarefiable iff 0 < n_s < 2^53.  Parameters: depth_step >= 1, num_depths J in [1, 256],
 *     J * depth_step <= 2^20; the depths are k_j = j * depth_step, j = 1 .. J.  Per sample (n = n_s) and integer m:
 *       Q(m, 0) = 1.0, and for k = 0, 1, ...: Q(m, k + 1) =
 *         +1.0 if m == 0 (an empty side gives exactly 1, not a product of roundings);
 *         +0.0 if m >= n - k (uint64 compare);
 *         (Q(m, k) * (double)(n - m - k)) * r_k otherwise, r_k = 1.0 / (double)(n - k).
 *     That is C(n - m, k) / C(n, k): the chance that none of k reads drawn without replacement is one of the m.
 *     For k_j <= n_s and each half branch x in {cb, cc}: miss = Q(x, k_j), all = Q(n - x, k_j) (the subtraction wraps),
 *       ru = 1.0 - miss,   uu = (1.0 - miss) - all, replaced by +0.0 unless uu > 0.0,
 *       term_u[b] = half[b] * (uu(cb) + uu(cc)),   term_r[b] the same with ru,
 *       curve[s][j] = {BS(term_u), BS(term_r)}: the expected unrooted and rooted PD of k_j reads.
 *     k_j > n_s, or a sample that is not rarefiable: {-1.0, -1.0}.  Every cell of every output is written.
 *
 * Edge correlation and edge dispersion (Czech et al. 2019; `gappa analyze correlation` and `dispersion`) of the cohort's
 *   samples: which branches' masses or imbalances go up and down with a column of per-sample metadata, and which vary
 *   across the samples at all.  From mass[S][N], first[N] and, for the correlation, meta[S][M], doubles, M in
 *   [1, EPIK_AMD_CORRELATION_MAX_COLUMNS = 64]; any NaN in meta means "missing", an infinity is refused with
 *   EPIK_AMD_ERR_INVALID.  No branch lengths are taken.  All arithmetic is IEEE double, every operation rounded on its
 *   own, nothing fused; + - * /, sqrt (correctly rounded), min, max and comparisons only.
 *   Used samples.  T_s, C_s[b], B_s[b] are exactly those of the KR rule.  Sample s is used iff T_s > 0.  Column c's set U_c
 *     is the used samples whose meta[s][c] is not NaN, in ascending s, indexed j = 0 .. L_c - 1.
 *   The two quantities of a branch: the mass xm_j[b] = (double)mass[s][b] / (double)T_s, and the imbalance
 *     xi_j[b] = (B_s[b] + C_s[b]) - 1.0 of the epca rule, for an inner b (first[b] < b).
 *   NA is the one bit pattern 0x7ff8000000000000 (EPIK_AMD_NA_BITS).  It is always written, never computed: no value that
 *     reaches an output is an arithmetic NaN, so the guards below come before the divisions.
 *   Pearson P(x, y) of two vectors over j = 0 .. L - 1:
 *       mx = (sequential sum of x from +0.0, j ascending) / (double)L,   my likewise,   dx_j = x_j - mx,   dy_j = y_j - my,
 *       sxx, syy, sxy = the sequential sums of dx * dx, dy * dy, dx * dy from +0.0, j ascending,
 *       den = sqrt(sxx) * sqrt(syy);      NA unless L >= 3 and den > 0.0, else min(max(sxy / den, -1.0), 1.0).
 *   Midranks: rank(x)_j = (double)#{i : x_i < x_j} + 0.5 * (double)(#{i : x_i == x_j} + 1), the second count with j itself.
 *     Exact half-integers, so an implementation may sort or count.  -0.0 == +0.0, as the comparison says.
 *   Per column c and branch b, over U_c, an epik_amd_correlation:
 *       mass_pearson = P(xm[b], y_c),   mass_spearman = P(rank(xm[b]), rank(y_c)),
 *       imbalance_pearson, imbalance_spearman: the same with xi; both NA where b is not inner (first[b] == b).
 *     used[c] = L_c.  An implementation may share out branches, columns and kinds, never the samples of one sum; it may
 *     reuse work between columns with the same U_c (mx, dx, sxx and the ranks of x do not depend on y).
 *   Dispersion, per branch over all used samples (L of them), an epik_amd_dispersion:
 *       mass_mean = mx,  mass_var = sxx / (double)L,  mass_sd = sqrt(mass_var),  mass_cv = mass_sd / mass_mean,
 *       mass_vmr = mass_var / mass_mean (both NA unless mass_mean > 0.0),  imbalance_mean, imbalance_var, imbalance_sd
 *       likewise (NA for a branch that is not inner).  All eight are NA when L = 0.
 *   Every cell of every output is written.  With cells that wrapped the values mean nothing, but they are still these bits.
 *
 * PERMANOVA (Anderson 2001; `adonis`) of the cohort's samples over the KR distances: are the groups of a factor column
 *   different?  From the matrix KR[S][S] of the KR rule, T_s, and labels[S][M], uint32, M in
 *   [1, EPIK_AMD_PERMANOVA_MAX_COLUMNS = 64]: a label is below EPIK_AMD_PERMANOVA_MAX_GROUPS = 256, 0xffffffff means
 *   "missing"; P = num_permutations in [1, 999 999] and a uint64 seed.  All arithmetic is IEEE double, every operation
 *   rounded on its own, nothing fused; + - * / and comparisons only.
 *   Used samples and groups.  Per column c, U_c is the samples with T_s > 0 and a label in c, in list order, L = |U_c|;
 *     positions 0 .. L - 1 index U_c.  The groups are the distinct labels in U_c, numbered by first appearance: G groups
 *     of sizes n_g; lambda_i is the group of position i.
 *   Squared distances.  A[i][j] = KR(u_i, u_j) * KR(u_i, u_j): one multiply of the KR doubles.  Symmetric bit for bit.
 *   The sums of a labelling mu.  Every sum is a sequential chain from +0.0:
 *       t_i = sum over j > i, ascending, with mu_j == mu_i, of A[i][j],
 *       W_g = sum over i, ascending, with mu_i == g, of t_i,
 *       SSW(mu) = sum over g, ascending, of W_g / (double)n_g      (each term a division).
 *     With every position in one group: r_i = t_i, T = W_0, and ss_total = T / (double)L.
 *     An implementation may share out rows, groups, permutations and tests; it may never split one chain.
 *   The observed test.  SSW_0 = SSW(lambda),  ss_within = SSW_0,  ss_among = ss_total - SSW_0,
 *       f = (ss_among / (double)(G - 1)) / (SSW_0 / (double)(L - G)),   r2 = ss_among / ss_total.
 *   Permutations.  For p = 1 .. P and position i, in uint64 arithmetic mod 2^64 (the splitmix64 finaliser of a counter):
 *       z = seed + (((uint64)p << 32) | i) * 0x9E3779B97F4A7C15,   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9,
 *       z = (z ^ z >> 27) * 0x94D049BB133111EB,                     key_p(i) = z ^ z >> 31.
 *     rank_p(i) = the number of positions whose (key, position) is smaller (the keys of one permutation never tie: the
 *     mix is a bijection; the position is in the rule anyway).  mu^p_i = lambda_{rank_p(i)}: the sizes do not change.
 *     Permutation 0 is the identity, mu^0 = lambda.
 *       at_most = #{p in 1 .. P : SSW(mu^p) <= SSW_0},     p = (double)(1 + at_most) / (double)(P + 1).
 *     ss_total is the same for every labelling, so SSW <= SSW_0 is the textbook's F >= F_0 without a division.
 *   Undefined.  G < 2 or L - G < 1: every double of the record is EPIK_AMD_NA_BITS and at_most = 0 (used = L and
 *     groups = G are still written).  SSW_0 == 0.0 or ss_total == 0.0: f is NA; ss_total == 0.0: r2 is NA; p is defined.
 *   Pairwise.  For groups g < h < EPIK_AMD_PERMANOVA_MAX_PAIR_GROUPS = 32 of a column: the same rule on the sub-list of
 *     U_c whose label is g or h, the positions renumbered inside it (the keys come from those positions), g before h as
 *     the two groups; undefined if n_g + n_h - 2 < 1.
 *   Results.  out[M][1 + Q], Q = EPIK_AMD_PERMANOVA_PAIR_SLOTS = 496 with pairwise and 0 without: slot 0 is the whole
 *     column, the pair (g, h) is slot 1 + h (h - 1) / 2 + g; a slot without a pair (h >= G) has used = groups = 0,
 *     at_most = 0 and NA doubles.  ssw[M][1 + Q][P + 1], where asked for: SSW(mu^p) for p = 0 .. P, NA for a test that is
 *     undefined or a slot without a pair.  group_ss[M][256], where asked for: W_g / (double)n_g of lambda for g < G of a
 *     column whose test is defined, NA otherwise.  Every cell of every output is written.
 *
 * Strata (blocked permutations; `strata =`, `how(blocks =)`): permute within strata only.  One rule for the four permutation
 *   tests (PERMANOVA, PERMDISP, the edge test, the sequential model), for a cohort whose samples are not exchangeable as a
 *   whole: a subject sampled several times, samples that come in batches.  strata[S], uint32, by sample: any value is a
 *   stratum id, there is no "missing" one.  A test has the positions 0 .. n - 1, its used samples in list order, as without
 *   strata; h_i is the stratum of the sample of position i, and key_p(i) is the PERMANOVA rule's.
 *       w_p(i) = the number of positions j with h_j == h_i whose (key_p(j), j) is smaller than (key_p(i), i),
 *       member(h, w) = the w-th position, ascending, among the positions of stratum h,
 *       sigma_p(i) = member(h_i, w_p(i)),       sigma_0 = the identity.
 *     Wherever a test uses rank_p(i) it uses sigma_p(i): mu^p_i = lambda_{sigma_p(i)} for PERMANOVA, PERMDISP and the edge
 *     test (a pairwise sub-list has its own positions, and the strata of their samples), and the model's row of Q.  sigma_p is
 *     a bijection that keeps every position in its stratum, so the sizes of the groups do not change and the labels of a
 *     stratum are the same multiset under every p.  With one stratum sigma_p = rank_p: the entries without strata, and strata
 *     == NULL, are this rule with h == 0 everywhere, and their bits are what they were.  Only the equality of ids enters:
 *     renumbering the strata changes no bit.  A factor that is constant inside every stratum cannot be permuted: every
 *     labelling is lambda, so every permuted statistic is the observed one and p = 1 (PERMDISP's permuted statistic is eta_r
 *     of the residuals, not eta2 of z: there every eta_r(mu^p) is eta_r(lambda)).
 *
 * Mantel, partial Mantel and ANOSIM (Mantel 1967, `mantel`; Smouse, Long & Sokal 1986, `mantel.partial`; Clarke 1993,
 *   `anosim`): does the distance between samples grow with the difference in a variable or with another distance, with a
 *   third held fixed; and are the ranked distances between groups larger than within them?  From the matrix D[S][S] of the
 *   chosen distance, T_s, P = num_permutations in [1, 999 999], a uint64 seed and, optionally, strata[S].  S is at most
 *   EPIK_AMD_MANTEL_MAX_SAMPLES = 8 192.  All arithmetic is IEEE double, every operation rounded on its own, nothing fused;
 *   + - * / sqrt and comparisons only.  NA is EPIK_AMD_NA_BITS, written and never computed.
 *   Sides.  values[Mv][S], Mv <= EPIK_AMD_MANTEL_MAX_COLUMNS = 64: side q < Mv is the column q of per-sample numbers, NaN
 *     means missing (an infinity is refused, and so is a column whose largest value less its smallest overflows, so every
 *     distance is finite); its distance is |v_s - v_t|, one subtraction and the absolute value.
 *     matrices[Mm][S][S] with matrix_present[Mm][S] (a byte a sample, 0: missing), Mm <= EPIK_AMD_MANTEL_MAX_MATRICES = 8:
 *     side Mv + k is matrix k, of which only the cells [s][t], s < t, are read (a cell between two present samples that is
 *     negative or not finite is refused).  Q = Mv + Mm >= 1.  methods: bit 0 pearson, bit 1 spearman, at least one.  control: a
 *     side, or EPIK_AMD_MANTEL_NO_CONTROL = 0xffffffff.  The tests are (side q, method) in side-major order, pearson before
 *     spearman: Q * popcount(methods) records.  With a control z every side q != z is tested with z held fixed (partial = 1);
 *     the control itself is tested plainly.
 *   List.  A test uses the samples with T_s > 0 that are present on its side and, if partial, on the control, in ascending
 *     s: the positions 0 .. n - 1, u_i the sample of position i.  The pairs are (i, j), i < j, i-major; m = n (n - 1) / 2.
 *   Triangle chain.  Every sum over the pairs is taken in two steps: t_i = the sequential chain over j = i + 1 .. n - 1,
 *     ascending, from +0.0; then the sequential chain of t_0 .. t_{n-2} from +0.0.  Rows may run in parallel; no chain is split.
 *   Values.  x(i, j) = D[u_i][u_j], y(i, j) the side's distance of (u_i, u_j), z(i, j) the control's, each for i < j (so
 *     s = u_i < t = u_j).  For spearman each of x, y, z is first replaced by its midranks among its own m values: less +
 *     (equal + 1) / 2, the correlation rule's two counts.
 *   Moments.  For a in x, y, z: mean_a = chain(a) / (double)m,  a' = a - mean_a,  ss_a = chain(a' * a').  For two of them
 *     s_ab = chain(a' * b')  and  r_ab = s_ab / sqrt(ss_a * ss_b).
 *   Statistic.  Plain: stat = r = r_xy; r_xz and r_yz are NA.  Partial: r = r_xy, r_xz, r_yz, and
 *       stat = (r_xy - r_xz * r_yz) / (sqrt(1.0 - r_xz * r_xz) * sqrt(1.0 - r_yz * r_yz)).
 *   Permutations.  For p = 1 .. P, sigma_p is the PERMANOVA rule's rank_p over the n positions, with strata the strata rule's
 *     sigma_p: the same shuffles for the same seed.  x'_p(i, j) = x'(sigma_p(i), sigma_p(j)) (x' is symmetric), s_xy and, if
 *     partial, s_xz are the chains over x'_p; the means, every ss and r_yz do not move.  stat_p is the statistic of these.  A
 *     partial permutation whose 1.0 - r_xz * r_xz is not > 0.0 has stat_p = NA and is not counted.
 *       at_least = #{p in 1 .. P : stat_p >= stat_0},     p = (double)(1 + at_least) / (double)(P + 1)     (one-sided).
 *   Undefined.  Unless n >= 3, ss_x != 0.0, ss_y != 0.0 and, if partial, ss_z != 0.0 and both radicands > 0.0: every double
 *     of the record is NA and at_least = 0 (used = n, side, method and partial are still written).
 *   Results.  out[Q * popcount(methods)] of epik_amd_mantel; stat[tests][P + 1], where asked for: stat_p for p = 0 .. P, NA for
 *     an undefined test.  Every cell of every output is written.
 *   ANOSIM.  Per column c of labels[S][M] (the PERMANOVA rule's labels, U_c, positions, groups by first appearance, G, n_g and
 *     lambda).  x is the midranks of D over the m pairs of the column's list.  lambda^p_i = lambda_{sigma_p(i)}, the PERMANOVA
 *     rule's labellings (sigma_p the strata rule's with strata).  W_p = the sum of x(i, j) over the pairs with lambda^p_i ==
 *     lambda^p_j; m_W = sum over g of n_g (n_g - 1) / 2, m_B = m - m_W.  Twice a midrank is an integer and every sum here is
 *     exact in a double (m (m + 1) < 2^53), so its order is free.
 *       mean_within_p = W_p / (double)m_W,   mean_between_p = ((double)(m (m + 1) / 2) - W_p) / (double)m_B,
 *       R_p = (mean_between_p - mean_within_p) / ((double)m / 2.0),
 *       at_least = #{p in 1 .. P : R_p >= R_0},     p = (double)(1 + at_least) / (double)(P + 1).
 *     The record has r = R_0, mean_between and mean_within of p = 0.  Defined iff G >= 2 and m_W >= 1; otherwise every double is
 *     NA and at_least = 0 (used = L and groups = G are still written).  out[M] of epik_amd_anosim; stat[M][P + 1], where asked
 *     for: R_p, NA for an undefined column.
 *
 * Edge model (a sequential linear model per branch by permutation, with the edge test's single-step max-statistic adjustment):
 *   on which branches does a term still matter once the terms before it are accounted for?  From mass[S][N], first[N] and the
 *   design exactly as the sequential model takes it (kind[T], labels[S][T], values[S][T], at most 16 terms and 64 columns),
 *   P = num_permutations in [1, 999 999], a uint64 seed and, optionally, strata[S].  All arithmetic is IEEE double, every
 *   operation rounded on its own, nothing fused; + - * / and comparisons only (the basis takes the model's sqrt).  NA is
 *   EPIK_AMD_NA_BITS, written and never computed.
 *   Samples, columns and basis.  U, L, the centred columns, the accepted columns q_c, df_k, R, `aliased` and df_res = L - 1 - R
 *     are the steps 1, 3 and 4 of the sequential model's rule, word for word: none depends on the response, so for the same
 *     design used, columns, rank, df and the aliased bytes equal the model's.
 *   Families.  Two vectors x over the positions of a branch b: f = 0 is xm[b], the mass of the correlation rule; f = 1 is
 *     xi[b], the imbalance (inner branches only).  mx, d_i and sxx are the edge test's chains.  There are no rank families.
 *   The sums of an arrangement sigma.  sigma_p is the PERMANOVA rule's rank_p among the L positions, with strata the strata
 *     rule's sigma_p; sigma_0 is the identity.  The response stays and whole rows of Q move, as in the model.
 *       s_c = the sequential sum from +0.0 over i ascending of q_c[sigma(i)] * d_i       (a product, then an addition),
 *       SS_k = the chain from +0.0 of s_c * s_c over the accepted columns of term k in order,
 *       SS_model = the chain from +0.0 of SS_k over the terms in order,       SS_res = sxx - SS_model.
 *     An implementation may share out terms, branches, families, permutations and columns; it may never split one chain.
 *   Statistic.  phi_k(sigma) = SS_k / (SS_k + SS_res) where SS_res > 0.0; otherwise 1.0 if SS_k > 0.0 and +0.0 if not (the
 *     conservative side).  phi is the partial R2, which increases with F_k at fixed degrees of freedom; it is bounded, so a
 *     maximum over branches compares like with like, and never below +0.0, so that maximum is one of bit patterns.
 *   Defined.  (b, f, k) is defined iff df_k >= 1, df_res >= 1, sxx > 0.0 and, for f = 1, b is inner.
 *   Observed (sigma_0).  ss = SS_k,  r2 = SS_k / sxx,  partial_r2 = phi_k,  f = (SS_k / (double)df_k) / (SS_res / (double)df_res),
 *     NA unless SS_res > 0.0;  sign = +1, -1 or 0, the sign of s_c, for a term with exactly one accepted column, 0 otherwise.
 *   p-values.  at_least = #{p in 1 .. P : phi_k(sigma_p) >= phi_k(sigma_0)},   p = (double)(1 + at_least) / (double)(P + 1);
 *       Mmax_p[k][f] = the maximum of phi_k(sigma_p) over the branches on which (b, f, k) is defined,
 *       max_at_least = #{p in 1 .. P : Mmax_p >= phi_k(sigma_0)},   p_adj = (double)(1 + max_at_least) / (double)(P + 1).
 *   Results.  out[T][N] of epik_amd_edgemodel, two families each: an undefined family has NA doubles, counts 0, sign 0.
 *     info: used = L, terms = T, columns = C, rank = R, df_res, df[k] and term_columns[k] for k < T, 0 beyond.  aliased[64] as
 *     the model's.  stat[T][2][N][P + 1], where asked for: phi_k(sigma_p), NA where undefined.  max[T][2][P + 1], where asked
 *     for: Mmax_p with p = 0 as well, NA where no branch is defined.  Every cell is written.
 *   By hand: four samples, the factor (a, a, b, b) and then the covariate (0, 1, 2, 3): q_0 = (-1/2, -1/2, 1/2, 1/2) and
 *     q_1 = (-1/2, 1/2, -1/2, 1/2).  A branch with d = q_0: sxx = 1, SS_1 = 1, SS_2 = 0, SS_res = 0: r2 = 1 and 0, partial_r2 = 1
 *     and +0.0, f NA, sign +1 and 0.  A branch with d = q_1: the same with the terms exchanged.  (The shares of a sample sum to one, so
 *     two branches of one cohort cannot both hold these deviations: the tests' case has d = q_0 / 2 on one branch and q_1 / 2 on
 *     another, sxx = 1/4, SS = 1/4 and 0, and r2, partial_r2 and the signs as here.)
 *
 * Principal coordinates (Gower 1966; classical scaling, `cmdscale`, `pcoa`) of the cohort's samples over the KR distances:
 *   the ordination in which beta diversity is drawn.  From the matrix KR[S][S] of the KR rule, T_s and K in [1, 64].  The KR
 *   distance on a tree is not Euclidean, so the doubly centred matrix may be indefinite: the negative eigenvalues are
 *   written out, never hidden.  All arithmetic is IEEE double, every operation rounded on its own, nothing fused.
 *   Used samples.  Sample s is used iff T_s > 0; the used samples, in ascending s, get the indices j = 0 .. L - 1 (u_j is
 *     the sample of index j).  L may be 0.
 *   Squares.  A2[i][j] = KR(u_i, u_j) * KR(u_i, u_j): one multiply, the PERMANOVA rule's squared distances.  The matrix is
 *     symmetric bit for bit as kr_device writes it.  For a forged one: r_i reads KR[u_j][u_i], and B[i][j], i <= j, reads
 *     KR[u_i][u_j]; the device, the host mirror (_pcoa_kr_host) and the tests' restatement all read those elements.
 *   Centring (Gower).  Every sum is a sequential chain from +0.0:
 *       r_i = (sum over j = 0 .. L - 1, ascending, of A2[i][j]) / (double)L,     g = (sum over i ascending of r_i) / (double)L,
 *       for i <= j: B[i][j] = -0.5 * (((A2[i][j] - r_i) - r_j) + g),  and B[j][i] = B[i][j].
 *     scale = max over j of |B[j][j]| (+0.0 for L = 0); trace = the sequential sum of B[j][j], j ascending, from +0.0;
 *     tol = 2^-52 * scale.
 *   Eigen-decomposition.  Exactly the Jacobi paragraph of the edge-PCA rule with A = B and this tol: the same rounds, the
 *     same three phases, the 64-sweep cap, `sweeps` and `converged`.
 *   Components.  mu_j = A[j][j], ordered by (mu descending, j ascending): mu[k], k = 0 .. L - 1, ALL L eigenvalues, the
 *     negative ones included; mu[k] = +0.0 for k >= L.  K' = min(K, L).  Axis k < K' is real iff mu_k > 2^-40 * scale.
 *     For a real axis, with j(k) the column of V it came from: j* = the first j with the largest |V[j][j(k)]|,
 *     sign = -1 iff V[j*][j(k)] < 0, else +1, and
 *       coord[s][k] = sign * (V[j(s)][j(k)] * sqrt(mu_k)).
 *     coord is +0.0 for an axis that is not real, for k >= K' and for an unused s.
 *     pos = the sequential sum from +0.0, k ascending, of the mu_k > 2^-40 * scale; neg = the same sum of the
 *     mu_k < -(2^-40 * scale) (so neg <= 0).  An eigenvalue in neither sum is `null`.
 *   The file derives, one division each: fraction_k = mu_k / pos, 0 when pos is 0; negative = -neg / pos, 0 when pos is 0:
 *     how far the cohort is from Euclidean.  Every cell of every output is written.
 *
 * Edge test (per-branch one-way ANOVA and Kruskal-Wallis by permutation, with the single-step max-statistic adjustment of
 *   Westfall & Young 1993): on which branches do the groups of a factor column differ?  From mass[S][N], first[N] and
 *   labels[S][M] as for PERMANOVA, M in [1, 64], but a label is below EPIK_AMD_EDGETEST_MAX_GROUPS = 32 (0xffffffff means
 *   "missing"); P = num_permutations in [1, 999 999] and a uint64 seed.  All arithmetic is IEEE double, every operation
 *   rounded on its own, nothing fused; + - * / and comparisons only.  NA is EPIK_AMD_NA_BITS, written and never computed.
 *   Samples and groups.  U_c, L, the positions, the groups by first appearance, G, n_g and lambda are exactly those of the
 *     PERMANOVA rule: the same for every branch of a column.
 *   Labellings.  mu^p, p = 0 .. P, is exactly the PERMANOVA rule's labelling of U_c: the same keys from the same seed, the
 *     same ranking, mu^0 = lambda.  A column tested with the same seed under both rules sees the same relabellings.
 *   Families.  Four vectors x over the positions of a branch b, f = 0 .. 3: xm[b], the mass of the correlation rule;
 *     rank(xm[b]), its midranks over U_c by the correlation rule; xi[b], the imbalance (inner branches only); rank(xi[b]).
 *   Sums.  mx = (sequential sum of x from +0.0, i ascending) / (double)L,   d_i = x_i - mx,
 *       sxx = the sequential sum of d_i * d_i from +0.0, i ascending;  for a labelling mu:
 *       S_g = the sequential sum from +0.0 over i ascending with mu_i == g of d_i,
 *       A(mu) = the sequential sum from +0.0 over g ascending of (S_g * S_g) / (double)n_g,     eta(mu) = A(mu) / sxx.
 *     An implementation may share out columns, branches, families, labellings and groups; it may never split one chain.
 *     (No S_g is ever -0.0: a chain from +0.0 cannot reach it.  So adding +0.0 to a chain changes nothing.)
 *   Defined.  A family of a branch is defined iff G >= 2, L - G >= 1 and sxx > 0.0 and, for f = 2 and 3, b is inner.
 *     (sxx is the computed double: identical values whose running sum rounds leave deviations of an ulp and count as varying.)
 *   Observed.  eta2 = eta(lambda).  f = 0 and 2: ssw = sxx - A(lambda),
 *       stat = (A(lambda) / (double)(G - 1)) / (ssw / (double)(L - G)), the one-way ANOVA F, NA unless ssw > 0.0.
 *     f = 1 and 3: stat = (double)(L - 1) * eta2, the Kruskal-Wallis H with its tie correction (SSA / SST of midranks).
 *   Permutation p-values.  at_least = #{p in 1 .. P : eta(mu^p) >= eta2},   p = (double)(1 + at_least) / (double)(P + 1);
 *       Mmax_p = the maximum over the defined branches of family f in column c of eta_b(mu^p)   (every eta is >= +0.0, so
 *       a maximum over the bit patterns is exact whatever the order),
 *       max_at_least = #{p in 1 .. P : Mmax_p >= eta2},   p_adj = (double)(1 + max_at_least) / (double)(P + 1).
 *   Direction.  top_mass and top_imbalance: the group g with the largest S_g / (double)n_g of lambda in family 0 and in
 *     family 2, the lowest g of a tie; 0xffffffff where that family is undefined.
 *   An undefined family: its doubles are NA and its counts 0.  used = L and groups = G are always written.
 *   Results.  out[M][N] records.  stat[M][4][N][P + 1], where asked for: eta(mu^p), NA where undefined.  max[M][4][P + 1],
 *     where asked for: Mmax_p with p = 0 as well, NA for a family without a defined branch.  Every cell is written.
 *
 * PERMDISP (Anderson 2006; vegan's `betadisper` + `permutest`, centroids) of the cohort's samples over the KR distances: do the
 *   groups of a factor column differ in spread?  The companion of a significant PERMANOVA, which cannot tell a difference in
 *   location from one in dispersion.  From the matrix KR[S][S], T_s, labels[S][M] (a label below 32, the edge test's cap, or
 *   0xffffffff), P in [1, 999 999] and a uint64 seed.  All arithmetic is IEEE double, every operation rounded on its own.
 *   U_c, the positions, the groups by first appearance, G, n_g, lambda, the labellings mu^p (the same keys from the same seed,
 *     mu^0 = lambda) and A2 = KR * KR are exactly those of the PERMANOVA rule.  A2[i][j] below is read as the square of
 *     KR[u_j][u_i] (the matrix is symmetric bit for bit as kr_device writes it; a forged matrix must be too).
 *   Distances to centroids, per column, in closed form (no eigenvectors: betadisper's "real-axes distance^2 minus
 *     imaginary-axes distance^2").  With W_g the PERMANOVA chain of group g under lambda:
 *       c_g = (W_g / (double)n_g) / (double)n_g,
 *       m_i = (the sequential sum from +0.0 over the positions j of the group g of i, ascending, j = i included, of
 *              A2[i][j]) / (double)n_g,       z2_i = m_i - c_g,      z_i = z2_i > 0.0 ? sqrt(z2_i) : +0.0,
 *       mean_g = (the sequential sum from +0.0 of z_i over the positions of g, ascending) / (double)n_g,  r_i = z_i - mean_g.
 *     A position with z2_i < 0.0 is `clipped` (vegan sets those to zero with a warning).  z, mean and r are those of the
 *     whole column whatever test uses them: a centroid does not depend on the other groups.
 *   A test is a list of n positions of the column in ascending order with G groups: the whole column, or, pairwise, for
 *     groups g < h < 32 the positions of g or h, renumbered 0 .. n - 1 (the keys come from those numbers), g before h.
 *   Observed.  The edge-test rule's sums over the test's positions with x = z: mx, d, sxx, S_g of lambda, A(lambda);
 *       eta2 = A(lambda) / sxx,  ssw = sxx - A(lambda),  f = (A(lambda) / (double)(G - 1)) / (ssw / (double)(n - G)), NA
 *       unless ssw > 0.0.  The test is defined iff G >= 2, n - G >= 1 and sxx > 0.0.
 *   Permutations of residuals (permutest.betadisper).  The edge-test rule's sums with x = r give eta_r(mu) = A_r(mu) / sxx_r;
 *       at_least = #{p in 1 .. P : eta_r(mu^p) >= eta2},     p = (double)(1 + at_least) / (double)(P + 1).
 *     F increases with eta at fixed (G, n): the textbook's F_p >= F_0 without a division.  If sxx_r is not > 0.0 there is
 *     nothing to permute: at_least = P, p = 1, and every permuted statistic is written as eta2 (a tie).
 *   Results.  out[M][1 + Q] of epik_amd_permdisp in the PERMANOVA slot layout (Q = 496 with pairwise, 0 without): used = n,
 *     groups = G and clipped (the clipped positions of the test) are always written, 0 for a slot without a pair; an
 *     undefined test has at_least = 0 and NA doubles.  stat[M][1 + Q][P + 1], where asked for: eta2 in slot 0, eta_r(mu^p) in
 *     slot p, NA for an undefined test.  group_mean[M][32]: mean_g for g < G, NA beyond.  z[M][S]: z of the sample's
 *     position, NA for a sample outside U_c.  Both for every column, defined or not.  Every cell of every output is written.
 *
 * Sequential model (McArdle & Anderson 2001; vegan's `adonis2(D ~ a + b + c, by = "terms")`): do the samples still differ by
 *   a term once the terms before it are accounted for?  From the matrix KR[S][S] (or another distance), T_s, and a design of
 *   T terms in [1, EPIK_AMD_MODEL_MAX_TERMS = 16] in test order: kind[T] (0 a factor, 1 numeric), labels[S][T] (uint32, a
 *   factor's label below EPIK_AMD_MODEL_MAX_GROUPS = 32, 0xffffffff missing; ignored for a numeric term), values[S][T]
 *   (double, NaN missing, never infinite; ignored for a factor); P in [1, 999 999] and a uint64 seed.  All arithmetic is IEEE
 *   double, every operation rounded on its own (+ - * / sqrt), nothing fused; every sum is a sequential chain from +0.0.
 *   The design may have EPIK_AMD_MODEL_MAX_COLUMNS = 64 columns at the most, counted on the arguments as given whatever the
 *   used samples: a numeric term counts 1, a factor the number of its distinct labels over all S samples less one (0 for none).
 *   1 Used samples.  U is the samples with T_s > 0 and a value for EVERY term (complete cases), in list order, L = |U|;
 *     positions 0 .. L - 1 index U.  A factor's groups are its distinct labels in U numbered by first appearance, G of them.
 *   2 Gower matrix.  B[L][L] over U exactly as the centring paragraph of the principal coordinates forms it (A2 one multiply,
 *     r_i, g, B[i][j] for i <= j and mirrored).  ss_total = the chain of B[i][i], i ascending (+0.0 for L = 0).
 *   3 Columns, in term order: a numeric term gives one column of its values; a factor term gives G - 1 columns (none for
 *     G = 0), the indicators (1.0 or 0.0) of the groups 1 .. G - 1, group 0 the baseline.  C columns in all.  Each is centred:
 *       mean = (chain over i ascending of x_i) / (double)L,   x_i = x_i - mean,   n0 = chain of x_i * x_i.
 *     (L = 0: no mean is formed, n0 = +0.0.)
 *   4 Basis, classical Gram-Schmidt twice.  For each column v in order, with q_0 .. q_{m-1} the columns accepted so far, two
 *     times over: h_k = chain over i ascending of q_k[i] * v[i] for every k (all from the same v), then
 *     v[i] = (..((v[i] - h_0 * q_0[i]) - h_1 * q_1[i]) ..), k ascending.  Then n1 = chain of v[i] * v[i].  The column is
 *     accepted iff n0 > 0.0 and n1 > 2^-40 * n0 (one multiply), and then q_m[i] = v[i] / sqrt(n1), a division each; otherwise
 *     it is aliased and dropped (a constant column, a covariate given twice, a factor nested in an earlier one).
 *     df_k = the accepted columns of term k,  R = their number in all,  df_res = L - 1 - R (an int64; may be negative).
 *   5 The sums of squares of an arrangement sigma of the positions (Q_sigma[i] = the row of Q at position sigma(i)):
 *       t_c[i] = chain over j = 0 .. L - 1 ascending of B[i][j] * q_c[sigma(j)]      (the full row; symmetry is not used),
 *       s_c = chain over i ascending of q_c[sigma(i)] * t_c[i],      SS_k = chain of s_c over the accepted columns of term k
 *       in order (+0.0 for none),   SS_model = chain of SS_k over the terms in order,   SS_res = ss_total - SS_model,
 *       F_k = (SS_k / (double)df_k) / (SS_res / (double)df_res),   R2_k = SS_k / ss_total,
 *     and for the whole model the same with SS_model and R.  A sigma whose SS_res is not > 0.0 has F = +infinity.
 *   6 Permutations.  sigma_p(i) = rank_p(i) of the PERMANOVA rule among the L positions: the same keys from the same seed,
 *     so both rules see the same shuffles.  Whole rows of Q move, B stays.  sigma_0 is the identity.
 *   7 Counts.  at_least_k = #{p in 1 .. P : F_k(sigma_p) >= F_k(sigma_0)} (B is indefinite for a tree distance, so SS_res of
 *     a permutation may fail to be > 0.0: its +infinity counts, the conservative side);  p = (double)(1 + at_least) / (double)(P + 1).
 *   8 Results.  out[T + 1] of epik_amd_model_term, the terms and then the whole model (df = R, columns = C): df and columns
 *     are always written.  df = 0: the doubles are NA and at_least = 0.  Otherwise ss is written, r2 unless ss_total is not
 *     > 0.0 (NA), and f, at_least and p unless df_res < 1 or the observed SS_res is not > 0.0 (NA, 0, NA).
 *     info: used = L, terms = T, columns = C, rank = R, df_res, ss_total, ss_res (the observed one).
 *     stat[T + 1][P + 1], where asked for: F of sigma_p, p = 0 the observed one; NA for a record whose f is NA.
 *     aliased[64]: 1 for a column that was dropped, in column order, 0 otherwise and beyond C.  Every cell is written.
 *   By hand: four samples at 0, 1, 2, 3 on a line, the factor (a, a, b, b) and then the covariate (0, 1, 2, 3): ss_total = 5,
 *     q_0 = (-1/2, -1/2, 1/2, 1/2) and SS_1 = 4, q_1 = (-1/2, 1/2, -1/2, 1/2) and SS_2 = 1, SS_res = 0: both F are NA, R2 = 0.8
 *     and 0.2.  The factor alone: SS_res = 1, F = 8, R2 = 0.8, PERMANOVA's numbers for that column.
 *
 * An epik_amd_cohort is an object of its own, created for a placer's device, num_branches and keep_at_most (whole
 * databases only, not a k-mer-space shard) and num_samples >= 1; all zero at create() and after reset().
 *   add_device  asynchronous on `stream`, allocates nothing: as epik_amd_profile_add_device, with d_samples (uint32 [n],
 *               device memory, required).  Reads of one sample that lie together are summed in LDS first (info:
 *               lds_path, the profile's limits and EPIK_AMD_PROFILE_LDS); any order is correct.
 *   read        synchronises the device, then copies out mass[S][N], best[S][N], totals[S] and bad_samples (each may be
 *               NULL).   add_cells: host arrays of those shapes (each may be NULL) added in -- merging devices.
 *   kr_device   checks the tree (the cohort's device and N) and the lengths (HOST float64 [N]), synchronises the device,
 *               copies the lengths, then enqueues the normalise and distance kernels on `stream`: d_out is float64
 *               [S][S] in device memory, every cell written.  The first call allocates the workspace.   kr: the same
 *               into host memory, synchronous.
 *   kr_host     the rule on the host from mass[S][N] and first[N], no device at all; first[b] > b is refused.
 *   unifrac_device  the checks of kr_device with its messages (tree, device, N, a negative or non-finite length names its
 *               branch), and metric outside 1 .. 3 (EPIK_AMD_DISTANCE_UNWEIGHTED, _WEIGHTED, _GENERALIZED) is refused with a
 *               message that names it.  Synchronises the device, copies the lengths, then enqueues ONE normalisation and the
 *               distance kernel on `stream` in kr_device's workspace: d_out is float64 [S][S] in device memory, every cell
 *               written.  The cells and a d_kr computed earlier are not changed.  Afterwards the cohort counts as
 *               normalised: permanova_device, pcoa_device and permdisp_device take d_out as they take kr_device's matrix.
 *               unifrac: the same into host memory, synchronous.
 *   unifrac_host  the rule on the host from mass[S][N], first[N] and branch_length[N], no device; first[b] > b is refused.
 *   permanova_metric / pcoa_metric / permdisp_metric: permanova, pcoa and permdisp with `metric` (EPIK_AMD_DISTANCE_KR or one
 *               of the three above; any other is refused with a message that names it) after branch_length: they run
 *               kr_device or unifrac_device themselves and hand the matrix on.  permanova, pcoa and permdisp are these with
 *               EPIK_AMD_DISTANCE_KR.  permanova_metric_host / pcoa_metric_host / permdisp_metric_host: the host mirrors
 *               likewise, kr_host or unifrac_host and then the *_kr_host entry.
 *   squash_device  checks and workspace as kr_device (the first call allocates a distance matrix of its own beside it),
 *               then enqueues the normalise and distance kernels and all S - 1 steps on `stream`, no readback in
 *               between: d_merges is epik_amd_squash_merge [S - 1] and d_num_merges one uint32 in device memory, every
 *               record written.  S = 1 is valid: zero merges (d_merges may be NULL then).  The cells are not changed.
 *               squash: the same into host memory, synchronous.
 *   squash_host the rule on the host, as kr_host.
 *   epca_device checks the tree as kr_device (no lengths) and K in [1, 64]; the first call allocates a workspace of its
 *               own, kept until destroy(): about 24 * S^2 + 8 * N * Sp bytes (three S x S matrices and the centred
 *               plane; Sp = S rounded up to 32), sized by S whatever the number of used samples.  d_mu float64 [K], d_proj float64 [S][K], d_edge float64 [K][N] and d_info one epik_amd_epca_info, all
 *               in device memory, every cell written.  It synchronises `stream` once for the number of used samples
 *               and, beyond 64 of them (the eigensolver's global path; EPIK_AMD_EPCA_LDS=0, read at the call, forces it),
 *               once per sweep for the sweep's rotation counter; the results are enqueued on `stream`.  The cells are
 *               not changed.   epca: the same into host memory, synchronous.
 *   epca_host   the rule on the host from mass[S][N] and first[N], no device; first[b] > b is refused.
 *   kmeans_device  checks the tree and the lengths as kr_device, K in [1, 64] and max_iterations in [1, 1000]; the first
 *               call allocates a workspace of its own, kept until destroy(): about 16 * N * 64 + 8 * S * 64 bytes (the
 *               centroid planes and D).  d_samples is epik_amd_kmeans_sample [S], d_clusters epik_amd_kmeans_cluster [K],
 *               d_centroids float64 [K][N] and d_info one epik_amd_kmeans_info, all in device memory, every cell written.
 *               The seeding is enqueued whole; then it synchronises `stream` once per iteration for `changed` (4 bytes
 *               each time); the results are enqueued on `stream`.  The cells are not changed.
 *               kmeans: the same into host memory, synchronous.
 *   kmeans_host the rule on the host from mass[S][N] and first[N], no device; first[b] > b is refused.
 *   alpha_device  checks the tree and the lengths as kr_device; the first alpha_device or rarefy_device allocates a
 *               workspace of its own, kept until destroy(): 16 * S * N + 8 * S bytes (cb, cc and n_s) and
 *               8 * S * ceil(N / 256) * max(5, 2 * 256) bytes of block partials.  d_alpha is epik_amd_alpha [S] in device
 *               memory, every cell written.  Once enqueued on `stream` it needs no readback.  The cells are not changed.
 *               alpha: the same into host memory, synchronous.
 *   alpha_host  the rule on the host from mass[S][N] and first[N], no device; first[b] > b is refused.
 *   rarefy_device  checks as alpha_device, depth_step >= 1, num_depths in [1, 256] and num_depths * depth_step <= 2^20;
 *               d_curve is float64 [S][J][2] in device memory, every cell written.  No readback; the cells are not changed.
 *               rarefy: the same into host memory, synchronous.
 *   rarefy_host the rule on the host from best[S][N] and first[N], no device; first[b] > b is refused.
 *   correlation_device  checks the tree as epca_device (its device and N), the nulls, num_columns in [1, 64] and meta
 *               (HOST, [S][M], read before the call returns) for an infinity.  The first correlation_device or
 *               dispersion_device allocates a workspace of its own, kept until destroy(): with Sp = S rounded up to 32,
 *               8 * N * Sp bytes (the masses, sample-fastest), 8 * Sp * (3 * 64 + 4 * 256) bytes (the columns, their
 *               deviations and ranks, and the general path's vectors of 256 workgroups), 4 * Sp * 65 bytes (the lists
 *               U_c) and under 4 KiB of tables.  d_out is epik_amd_correlation [M][N] and d_used uint32 [M] in device
 *               memory, every cell written.  Once enqueued on `stream` it needs no readback.  The cells are not changed.
 *               EPIK_AMD_CORRELATION_LDS=0, read at the call, forces the path that keeps a branch's vectors in global
 *               memory (taken anyway beyond 1 024 samples); the bits are the same.
 *               correlation: the same into host memory, synchronous.
 *   correlation_host  the rule on the host from mass[S][N], first[N] and meta[S][M], no device; first[b] > b is refused.
 *   dispersion_device  checks as correlation_device, takes no metadata; d_out is epik_amd_dispersion [N] in device memory,
 *               every cell written.  dispersion: the same into host memory, synchronous.
 *   dispersion_host  the rule on the host from mass[S][N] and first[N], no device; first[b] > b is refused.
 *   permanova_device  takes d_kr, float64 [S][S] in device memory as kr_device wrote it for the cells as they are (so T_s
 *               is in the cohort's workspace: a cohort whose kr_device never ran is refused), and labels (HOST [S][M],
 *               read before the call returns): refused are a null cohort, d_kr, labels or d_out, num_columns outside
 *               [1, 64], num_permutations outside [1, 999 999], a label in [256, 0xffffffff) and, with pairwise, a column
 *               with more than 32 distinct labels.  Synchronises the device, then the workspace (grown where a call needs
 *               more, kept until destroy(): with Sp = S rounded up to 32, 8 S^2 bytes of squared distances, 9 Sp bytes a
 *               column, or 164 Sp with pairwise, for the labels and the tests' lists, 44 bytes a test, 1 KiB a column, and
 *               44 Sp bytes for each of 256 workgroups of the general path).  d_out is epik_amd_permanova [M][1 + Q]; d_ssw (may be null) float64 [M][1 + Q][P + 1]; d_group_ss
 *               (may be null) float64 [M][256]; all in device memory.  Once enqueued on `stream` it needs no readback.
 *               The cells and d_kr are not changed.  A test of up to 1 024 positions keeps its labellings, keys and row
 *               sums in LDS; beyond, or with EPIK_AMD_PERMANOVA_LDS=0 (read at the call), in global memory: the same bits.
 *               permanova: runs kr_device itself (tree and lengths checked as there), the same into host memory,
 *               synchronous; ssw and group_ss may be null.
 *   permanova_host  the rule on the host from mass[S][N], first[N], branch_length[N] and the labels, no device.
 *               permanova_kr_host: the same from a matrix kr[S][S] and totals[S] (T_s; only > 0 matters).
 *   pcoa_device  takes d_kr as permanova_device does (so T_s is in the cohort's workspace: a cohort whose kr_device never
 *               ran is refused) and K in [1, 64]; refused are a null cohort, d_kr, d_mu, d_coord or d_info.  Synchronises
 *               the device, then the workspace of its own (allocated by the first call, kept until destroy(): about
 *               24 * S^2 + 40 * S bytes, three S x S matrices and the vectors).  d_mu float64 [S], d_coord float64 [S][K]
 *               and d_info one epik_amd_pcoa_info, all in device memory, every cell written.  It synchronises `stream`
 *               once for the number of used samples and, beyond 64 of them (the eigensolver's global path;
 *               EPIK_AMD_PCOA_LDS=0, read at the call, forces it), once per sweep for the sweep's rotation counter; the
 *               results are enqueued on `stream`.  The cells and d_kr are not changed.
 *               pcoa: runs kr_device itself (tree and lengths checked as there), the same into host memory, synchronous.
 *   pcoa_host   the rule on the host from mass[S][N], first[N] and branch_length[N], no device.
 *               pcoa_kr_host: the same from a matrix kr[S][S] and totals[S] (T_s; only > 0 matters).
 *   edgetest_device  checks the tree as correlation_device (its device and N) and labels (HOST [S][M], read before the call
 *               returns): refused are a null cohort, tree, labels or d_out, num_columns outside [1, 64], num_permutations
 *               outside [1, 999 999] and a label in [32, 0xffffffff).  It shares the workspace of correlation_device (the
 *               masses, sample-fastest) and keeps one of its own until destroy(), grown where a call needs more: with Sp = S
 *               rounded up to 32, 32 * N * Sp bytes (the four centred vectors of every branch), 32 * (P + 1) bytes (Mmax),
 *               1 024 * Sp bytes (a chunk of 1 024 labellings, a byte a position), 32 * Sp bytes for each of 256 workgroups
 *               of the general path, 9 * Sp bytes a column and 40 * N bytes of tables.  The columns run one after another
 *               in it, the permutations in chunks of 1 024.  d_out is epik_amd_edgetest [M][N]; d_stat (may be null) float64
 *               [M][4][N][P + 1]; d_max (may be null) float64 [M][4][P + 1]; all in device memory.  Once enqueued on
 *               `stream` it needs no readback.  The cells are not changed.  A column of up to 1 024 positions keeps a
 *               branch's vectors in LDS; beyond, or with EPIK_AMD_EDGETEST_LDS=0 (read at the call), in global memory:
 *               the same bits.   edgetest: the same into host memory, synchronous; stat and max may be null.
 *   edgetest_host  the rule on the host from mass[S][N], first[N] and the labels, no device; first[b] > b is refused.
 *   permdisp_device  takes d_kr and labels as permanova_device does (a cohort whose kr_device never ran is refused): refused
 *               are a null cohort, d_kr, labels, d_out, d_group_mean or d_z, num_columns outside [1, 64], num_permutations
 *               outside [1, 999 999] and a label in [32, 0xffffffff).  Synchronises the device, then a workspace of its own,
 *               grown where a call needs more and kept until destroy(): with Sp = S rounded up to 32 and lists = 32 with
 *               pairwise, 1 without, about 37 Sp bytes a column, 13 Sp * lists bytes of the tests' lists and residuals,
 *               1 024 Sp * lists bytes of a chunk of 1 024 labellings (a byte a position) and 64 bytes a test.  The columns
 *               run one after another in it, the permutations in chunks of 1 024.  d_out is epik_amd_permdisp [M][1 + Q];
 *               d_stat (may be null) float64 [M][1 + Q][P + 1]; d_group_mean float64 [M][32]; d_z float64 [M][S]; all in
 *               device memory.  Once enqueued on `stream` it needs no readback.  The cells and d_kr are not changed.
 *               permdisp: runs kr_device itself, the same into host memory, synchronous; stat may be null.
 *   permdisp_host  the rule on the host from mass[S][N], first[N], branch_length[N] and the labels, no device.
 *               permdisp_kr_host: the same from a matrix kr[S][S] and totals[S] (T_s; only > 0 matters).
 *   model_device  takes d_kr as permanova_device does (a cohort whose kr_device never ran is refused) and the design, kind[T],
 *               labels[S][T] and values[S][T] (HOST, read before the call returns): refused are a null cohort, d_kr, kind,
 *               labels, values, d_out, d_info or d_aliased, num_terms outside [1, 16], a kind other than 0 or 1,
 *               num_permutations outside [1, 999 999], a factor's label in [32, 0xffffffff), an infinite value of a numeric
 *               term and a design of more than 64 columns.  Synchronises the device, then a workspace of its own, grown where
 *               a call needs more and kept until destroy(): with Sp = S rounded up to 32, 8 S^2 bytes (B), 17 Sp bytes a term,
 *               528 Sp bytes (the basis Q, 64 columns wide, and two vectors) and, beyond 128 samples, 272 Sp bytes for each workgroup of
 *               the permutations, min(ceil(P / 4), 256, EPIK_AMD_MAX_BLOCKS) of them (the row sums of 4 permutations and 8
 *               columns, and their arrangements).  d_out is epik_amd_model_term [T + 1],
 *               d_info one epik_amd_model_info, d_stat (may be null) float64 [T + 1][P + 1], d_aliased 64 bytes; all in
 *               device memory.  Once enqueued on `stream` it needs no readback.  The cells and d_kr are not changed.  A
 *               design of up to 128 positions keeps the row sums and arrangements in LDS; beyond, or with
 *               EPIK_AMD_MODEL_LDS=0 (read at the call), in global memory: the same bits.
 *               model: runs kr_device itself, the same into host memory, synchronous; stat may be null.  model_metric: with
 *               `metric` as permanova_metric.
 *   model_host  the rule on the host from mass[S][N], first[N], branch_length[N] and the design, no device; model_metric_host
 *               with `metric`.  model_kr_host: the same from a matrix kr[S][S] and totals[S] (T_s; only > 0 matters).
 *   edgemodel_device  checks the tree as edgetest_device and the design as model_device (HOST, read before the call returns):
 *               refused are a null cohort, tree, kind, labels, values, d_out, d_info or d_aliased, and what model_device
 *               refuses of a design.  It shares the workspace of correlation_device (the masses) and keeps one of its own until
 *               destroy(), grown where a call needs more: with Sp = S rounded up to 32, 16 * N * Sp bytes (the two centred
 *               vectors of every branch), up to 49 152 * Sp bytes (the arranged basis and the arrangements of a chunk of
 *               permutations: 12 bytes a chain, min(P + 1, a chunk's permutations) times the design's columns of them, 4 096 at the most), 528 Sp bytes (the basis), 16 * T * (N + P + 1) bytes (the observed phi and Mmax),
 *               16 Sp bytes for each of 256 workgroups of the general path, 17 Sp bytes a term and 28 * N bytes of tables.
 *               d_out is epik_amd_edgemodel [T][N], d_info one epik_amd_edgemodel_info, d_aliased 64 bytes; d_stat (may be null)
 *               float64 [T][2][N][P + 1]; d_max (may be null) float64 [T][2][P + 1]; all in device memory.  Once enqueued on
 *               `stream` it needs no readback.  The cells are not changed.  A cohort of up to 1 024 samples keeps a branch's
 *               vectors in LDS in the observed pass; beyond, or with EPIK_AMD_EDGEMODEL_LDS=0 (read at the call), in global
 *               memory: the same bits.   edgemodel: the same into host memory, synchronous; stat and max may be null.
 *               _strata forms: with strata[S] (host; NULL: the bytes of the entry without it).
 *   edgemodel_host  the rule on the host from mass[S][N], first[N] and the design, no device; first[b] > b is refused.
 * cohort_reads / _strands / _frames / _mates: the profile_* twins with samples[n] (HOST uint32) beside the weights.
 */
typedef struct epik_amd_cohort epik_amd_cohort;
int epik_amd_cohort_create(const epik_amd_placer *p, uint32_t num_samples, epik_amd_cohort **out);
void epik_amd_cohort_destroy(epik_amd_cohort *cohort);
int epik_amd_cohort_reset(epik_amd_cohort *cohort);
int epik_amd_cohort_info(const epik_amd_cohort *cohort, uint32_t *num_samples, uint32_t *num_branches, uint32_t *lds_path);
int epik_amd_cohort_read(epik_amd_cohort *cohort, uint64_t *mass, uint64_t *best, epik_amd_profile_totals *totals,
                         uint64_t *bad_samples);
int epik_amd_cohort_add_cells(epik_amd_cohort *cohort, const uint64_t *mass, const uint64_t *best,
                              const epik_amd_profile_totals *totals);
int epik_amd_cohort_add_device(epik_amd_cohort *cohort, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                               const void *d_weights, const void *d_samples, uint64_t n, void *stream);
int epik_amd_cohort_kr_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_out,
                              void *stream);
int epik_amd_cohort_kr(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, double *out);
int epik_amd_cohort_kr_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                            const double *branch_length, double *out);
#define EPIK_AMD_DISTANCE_KR 0u
#define EPIK_AMD_DISTANCE_UNWEIGHTED 1u
#define EPIK_AMD_DISTANCE_WEIGHTED 2u
#define EPIK_AMD_DISTANCE_GENERALIZED 3u
int epik_amd_cohort_unifrac_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                   uint32_t metric, void *d_out, void *stream);
int epik_amd_cohort_unifrac(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                            double *out);
int epik_amd_cohort_unifrac_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                 const double *branch_length, uint32_t metric, double *out);
typedef struct epik_amd_squash_merge {
    uint32_t a, b;       /* the two nodes merged: a leaf is its sample, an internal node S + the step that made it */
    double dist;         /* D[r][c] when they were merged */
    double len_a, len_b; /* KR(merged, a), KR(merged, b): the edge lengths of the cluster tree */
} epik_amd_squash_merge; /* 32 bytes */
#define EPIK_AMD_SQUASH_NONE 0xffffffffu
int epik_amd_cohort_squash_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                  void *d_merges, void *d_num_merges, void *stream);
int epik_amd_cohort_squash(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                           epik_amd_squash_merge *merges, uint32_t *num_merges);
int epik_amd_cohort_squash_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, epik_amd_squash_merge *merges, uint32_t *num_merges);
typedef struct epik_amd_epca_info {
    uint32_t used, components; /* L, and K' = min(K, L) */
    uint32_t sweeps, converged;
    double trace, scale;
} epik_amd_epca_info; /* 32 bytes */
#define EPIK_AMD_EPCA_MAX_COMPONENTS 64u
#define EPIK_AMD_JACOBI_MAX_SWEEPS 64u /* the cap of the Jacobi paragraph, whoever uses it */
#define EPIK_AMD_EPCA_MAX_SWEEPS EPIK_AMD_JACOBI_MAX_SWEEPS
#define EPIK_AMD_PCOA_MAX_SWEEPS EPIK_AMD_JACOBI_MAX_SWEEPS
int epik_amd_cohort_epca_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, uint32_t num_components, void *d_mu,
                                void *d_proj, void *d_edge, void *d_info, void *stream);
int epik_amd_cohort_epca(epik_amd_cohort *cohort, const epik_amd_tree *tree, uint32_t num_components, double *mu,
                         double *proj, double *edge, epik_amd_epca_info *info);
int epik_amd_cohort_epca_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                              uint32_t num_components, double *mu, double *proj, double *edge, epik_amd_epca_info *info);
typedef struct epik_amd_kmeans_info {
    uint32_t used, clusters; /* L, and K' = min(K, L) */
    uint32_t iterations, converged;
} epik_amd_kmeans_info; /* 16 bytes */
typedef struct epik_amd_kmeans_sample {
    uint32_t cluster, zero; /* EPIK_AMD_KMEANS_NONE for a sample without mass */
    double dist;            /* KR(sample, its centroid) at the last assignment; -1.0 without mass */
} epik_amd_kmeans_sample; /* 16 bytes */
typedef struct epik_amd_kmeans_cluster {
    uint32_t size, seed;     /* its members; the sample that seeded it, EPIK_AMD_KMEANS_NONE for k >= K' */
    double sum_dist, sum_sq; /* over its members: dist, dist * dist */
} epik_amd_kmeans_cluster; /* 24 bytes */
#define EPIK_AMD_KMEANS_MAX_CLUSTERS 64u
#define EPIK_AMD_KMEANS_MAX_ITERATIONS 1000u
#define EPIK_AMD_KMEANS_NONE 0xffffffffu
int epik_amd_cohort_kmeans_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                  uint32_t num_clusters, uint32_t max_iterations, void *d_samples, void *d_clusters,
                                  void *d_centroids, void *d_info, void *stream);
int epik_amd_cohort_kmeans(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                           uint32_t num_clusters, uint32_t max_iterations, epik_amd_kmeans_sample *samples,
                           epik_amd_kmeans_cluster *clusters, double *centroids, epik_amd_kmeans_info *info);
int epik_amd_cohort_kmeans_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, uint32_t num_clusters, uint32_t max_iterations,
                                epik_amd_kmeans_sample *samples, epik_amd_kmeans_cluster *clusters, double *centroids,
                                epik_amd_kmeans_info *info);
typedef struct epik_amd_alpha {
    double pd, rooted_pd;       /* unrooted and rooted phylogenetic diversity */
    double bwpd_half, bwpd_one; /* balance-weighted PD at theta = 0.5 and 1 */
    double quadratic;           /* Rao's quadratic entropy */
} epik_amd_alpha; /* 40 bytes */
#define EPIK_AMD_DIVERSITY_BLOCK 256u
#define EPIK_AMD_RAREFY_MAX_DEPTHS 256u
#define EPIK_AMD_RAREFY_MAX_DEPTH (1u << 20)
int epik_amd_cohort_alpha_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                 void *d_alpha, void *stream);
int epik_amd_cohort_alpha(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                          epik_amd_alpha *alpha);
int epik_amd_cohort_alpha_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                               const double *branch_length, epik_amd_alpha *alpha);
int epik_amd_cohort_rarefy_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                  uint32_t depth_step, uint32_t num_depths, void *d_curve, void *stream);
int epik_amd_cohort_rarefy(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                           uint32_t depth_step, uint32_t num_depths, double *curve);
int epik_amd_cohort_rarefy_host(const uint64_t *best, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, uint32_t depth_step, uint32_t num_depths, double *curve);
typedef struct epik_amd_correlation {
    double mass_pearson, mass_spearman;
    double imbalance_pearson, imbalance_spearman; /* EPIK_AMD_NA_BITS for a branch that is not inner */
} epik_amd_correlation; /* 32 bytes */
typedef struct epik_amd_dispersion {
    double mass_mean, mass_var, mass_sd, mass_cv, mass_vmr;
    double imbalance_mean, imbalance_var, imbalance_sd;
} epik_amd_dispersion; /* 64 bytes */
#define EPIK_AMD_CORRELATION_MAX_COLUMNS 64u
#define EPIK_AMD_NA_BITS 0x7ff8000000000000ull
int epik_amd_cohort_correlation_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *meta,
                                       uint32_t num_columns, void *d_out, void *d_used, void *stream);
int epik_amd_cohort_correlation(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *meta, uint32_t num_columns,
                                epik_amd_correlation *out, uint32_t *used);
int epik_amd_cohort_correlation_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                     const double *meta, uint32_t num_columns, epik_amd_correlation *out, uint32_t *used);
int epik_amd_cohort_dispersion_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, void *d_out, void *stream);
int epik_amd_cohort_dispersion(epik_amd_cohort *cohort, const epik_amd_tree *tree, epik_amd_dispersion *out);
int epik_amd_cohort_dispersion_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                    epik_amd_dispersion *out);
typedef struct epik_amd_permanova {
    uint32_t used, groups; /* L and G of the test; 0, 0 for a slot without a pair */
    uint64_t at_most;      /* #{p >= 1 : SSW(mu^p) <= SSW_0} */
    double ss_total, ss_within, f, r2, p;
} epik_amd_permanova; /* 56 bytes */
#define EPIK_AMD_PERMANOVA_MAX_COLUMNS 64u
#define EPIK_AMD_PERMANOVA_MAX_GROUPS 256u
#define EPIK_AMD_PERMANOVA_MAX_PAIR_GROUPS 32u
#define EPIK_AMD_PERMANOVA_PAIR_SLOTS 496u
#define EPIK_AMD_PERMANOVA_MAX_PERMUTATIONS 999999u
#define EPIK_AMD_PERMANOVA_MISSING 0xffffffffu
int epik_amd_cohort_permanova_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, uint32_t num_columns,
                                     uint32_t num_permutations, uint64_t seed, int pairwise, void *d_out, void *d_ssw,
                                     void *d_group_ss, void *stream);
int epik_amd_cohort_permanova(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                              const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                              int pairwise, epik_amd_permanova *out, double *ssw, double *group_ss);
int epik_amd_cohort_permanova_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                   const double *branch_length, const uint32_t *labels, uint32_t num_columns,
                                   uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permanova *out, double *ssw,
                                   double *group_ss);
int epik_amd_cohort_permanova_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                     uint32_t metric, const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations,
                                     uint64_t seed, int pairwise, epik_amd_permanova *out, double *ssw, double *group_ss);
int epik_amd_cohort_permanova_metric_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches,
                                          const uint32_t *first, const double *branch_length, uint32_t metric,
                                          const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                                          int pairwise, epik_amd_permanova *out, double *ssw, double *group_ss);
int epik_amd_cohort_permanova_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                      uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                      epik_amd_permanova *out, double *ssw, double *group_ss);
/* The same with the strata rule: the _device, _metric, _metric_host and _kr_host entries plus strata[S] (host memory; NULL: the
 * bytes of the entry without it).  Refused as their siblings refuse.  Likewise for PERMDISP, the model and the edge test below. */
int epik_amd_cohort_permanova_strata_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, uint32_t num_columns,
                                            uint32_t num_permutations, uint64_t seed, int pairwise, void *d_out, void *d_ssw,
                                            void *d_group_ss, void *stream, const uint32_t *strata);
int epik_amd_cohort_permanova_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                     uint32_t metric, const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations,
                                     uint64_t seed, int pairwise, epik_amd_permanova *out, double *ssw, double *group_ss,
                                     const uint32_t *strata);
int epik_amd_cohort_permanova_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches,
                                          const uint32_t *first, const double *branch_length, uint32_t metric,
                                          const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                                          int pairwise, epik_amd_permanova *out, double *ssw, double *group_ss,
                                          const uint32_t *strata);
int epik_amd_cohort_permanova_strata_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples,
                                             const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations,
                                             uint64_t seed, int pairwise, epik_amd_permanova *out, double *ssw, double *group_ss,
                                             const uint32_t *strata);
/* Mantel, partial Mantel and ANOSIM (the rule above).  The sides, labels and strata are host memory (strata NULL: none; values
 * or matrices NULL with a count of 0); stat may be NULL.  _device: over d_dist, float64 [S][S] in device memory as kr_device or
 * unifrac_device wrote it for this cohort, into d_out and d_stat in device memory, asynchronous on `stream` once the sides are
 * copied, no readback.  The entry with tree and lengths runs the distance `metric` itself, synchronous, into host memory.
 * _host: the rule on the host from the cells; _kr_host: from a matrix and totals[S].  S > 8 192, a count outside its range, a
 * control that names no side, or a null pointer: EPIK_AMD_ERR_INVALID, nothing written. */
typedef struct epik_amd_mantel {
    uint32_t used, side, method, partial; /* n; the side q; 0 pearson, 1 spearman; 1 with the control held fixed */
    uint64_t at_least;                    /* #{p >= 1 : stat_p >= stat_0} */
    double r, r_xz, r_yz, stat, p;
} epik_amd_mantel; /* 64 bytes */
typedef struct epik_amd_anosim {
    uint32_t used, groups; /* L and G of the column */
    uint64_t at_least;     /* #{p >= 1 : R_p >= R_0} */
    double r, mean_between, mean_within, p;
} epik_amd_anosim; /* 48 bytes */
#define EPIK_AMD_MANTEL_MAX_SAMPLES 8192u
#define EPIK_AMD_MANTEL_MAX_COLUMNS 64u
#define EPIK_AMD_MANTEL_MAX_MATRICES 8u
#define EPIK_AMD_MANTEL_PEARSON 1u
#define EPIK_AMD_MANTEL_SPEARMAN 2u
#define EPIK_AMD_MANTEL_NO_CONTROL 0xffffffffu
int epik_amd_cohort_mantel_device(epik_amd_cohort *cohort, const void *d_dist, const double *values, uint32_t num_columns,
                                  const double *matrices, const uint8_t *matrix_present, uint32_t num_matrices, uint32_t methods,
                                  uint32_t control, uint32_t num_permutations, uint64_t seed, const uint32_t *strata, void *d_out,
                                  void *d_stat, void *stream);
int epik_amd_cohort_mantel(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                           const double *values, uint32_t num_columns, const double *matrices, const uint8_t *matrix_present,
                           uint32_t num_matrices, uint32_t methods, uint32_t control, uint32_t num_permutations, uint64_t seed,
                           const uint32_t *strata, epik_amd_mantel *out, double *stat);
int epik_amd_cohort_mantel_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, uint32_t metric, const double *values, uint32_t num_columns,
                                const double *matrices, const uint8_t *matrix_present, uint32_t num_matrices, uint32_t methods,
                                uint32_t control, uint32_t num_permutations, uint64_t seed, const uint32_t *strata,
                                epik_amd_mantel *out, double *stat);
int epik_amd_cohort_mantel_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const double *values,
                                   uint32_t num_columns, const double *matrices, const uint8_t *matrix_present,
                                   uint32_t num_matrices, uint32_t methods, uint32_t control, uint32_t num_permutations,
                                   uint64_t seed, const uint32_t *strata, epik_amd_mantel *out, double *stat);
int epik_amd_cohort_anosim_device(epik_amd_cohort *cohort, const void *d_dist, const uint32_t *labels, uint32_t num_columns,
                                  uint32_t num_permutations, uint64_t seed, const uint32_t *strata, void *d_out, void *d_stat,
                                  void *stream);
int epik_amd_cohort_anosim(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                           const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                           const uint32_t *strata, epik_amd_anosim *out, double *stat);
int epik_amd_cohort_anosim_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, uint32_t metric, const uint32_t *labels, uint32_t num_columns,
                                uint32_t num_permutations, uint64_t seed, const uint32_t *strata, epik_amd_anosim *out,
                                double *stat);
int epik_amd_cohort_anosim_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                   uint32_t num_columns, uint32_t num_permutations, uint64_t seed, const uint32_t *strata,
                                   epik_amd_anosim *out, double *stat);
typedef struct epik_amd_pcoa_info {
    uint32_t used, components; /* L, and K' = min(K, L) */
    uint32_t sweeps, converged;
    double trace, scale;
    double pos, neg;           /* the sums of the eigenvalues above 2^-40 * scale and below its negative */
} epik_amd_pcoa_info; /* 48 bytes */
#define EPIK_AMD_PCOA_MAX_COMPONENTS 64u
int epik_amd_cohort_pcoa_device(epik_amd_cohort *cohort, const void *d_kr, uint32_t num_components, void *d_mu, void *d_coord,
                                void *d_info, void *stream);
int epik_amd_cohort_pcoa(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                         uint32_t num_components, double *mu, double *coord, epik_amd_pcoa_info *info);
int epik_amd_cohort_pcoa_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                              const double *branch_length, uint32_t num_components, double *mu, double *coord,
                              epik_amd_pcoa_info *info);
int epik_amd_cohort_pcoa_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                uint32_t num_components, double *mu, double *coord, epik_amd_pcoa_info *info);
int epik_amd_cohort_pcoa_metric_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                     const double *branch_length, uint32_t metric, uint32_t num_components, double *mu,
                                     double *coord, epik_amd_pcoa_info *info);
int epik_amd_cohort_pcoa_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, uint32_t num_components,
                                 double *mu, double *coord, epik_amd_pcoa_info *info);
typedef struct epik_amd_edgetest_family {
    double eta2, stat, p, p_adj;        /* stat: F for the families 0 and 2, H for 1 and 3 */
    uint64_t at_least, max_at_least;    /* #{p >= 1 : eta(mu^p) >= eta2}, #{p >= 1 : Mmax_p >= eta2} */
} epik_amd_edgetest_family; /* 48 bytes */
typedef struct epik_amd_edgetest {
    uint32_t used, groups;              /* L and G of the column */
    epik_amd_edgetest_family family[4]; /* mass, rank(mass), imbalance, rank(imbalance) */
    uint32_t top_mass, top_imbalance;   /* the group with the largest mean of family 0 and 2; 0xffffffff where undefined */
} epik_amd_edgetest; /* 208 bytes */
#define EPIK_AMD_EDGETEST_MAX_COLUMNS 64u
#define EPIK_AMD_EDGETEST_MAX_GROUPS 32u
#define EPIK_AMD_EDGETEST_FAMILIES 4u
#define EPIK_AMD_EDGETEST_MAX_PERMUTATIONS 999999u
#define EPIK_AMD_EDGETEST_MISSING 0xffffffffu
int epik_amd_cohort_edgetest_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels,
                                    uint32_t num_columns, uint32_t num_permutations, uint64_t seed, void *d_out, void *d_stat,
                                    void *d_max, void *stream);
int epik_amd_cohort_edgetest(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels, uint32_t num_columns,
                             uint32_t num_permutations, uint64_t seed, epik_amd_edgetest *out, double *stat, double *max);
int epik_amd_cohort_edgetest_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                  const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                                  epik_amd_edgetest *out, double *stat, double *max);
int epik_amd_cohort_edgetest_strata_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels,
                                           uint32_t num_columns, uint32_t num_permutations, uint64_t seed, void *d_out,
                                           void *d_stat, void *d_max, void *stream, const uint32_t *strata);
int epik_amd_cohort_edgetest_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels,
                                    uint32_t num_columns, uint32_t num_permutations, uint64_t seed, epik_amd_edgetest *out,
                                    double *stat, double *max, const uint32_t *strata);
int epik_amd_cohort_edgetest_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                         const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                                         epik_amd_edgetest *out, double *stat, double *max, const uint32_t *strata);
typedef struct epik_amd_permdisp {
    uint32_t used, groups; /* n and G of the test; 0, 0 for a slot without a pair */
    uint32_t clipped, pad; /* the positions of the test with z2 < 0; pad is 0 */
    uint64_t at_least;     /* #{p >= 1 : eta_r(mu^p) >= eta2} */
    double eta2, f, p;
} epik_amd_permdisp; /* 48 bytes */
#define EPIK_AMD_PERMDISP_MAX_COLUMNS 64u
#define EPIK_AMD_PERMDISP_MAX_GROUPS 32u
#define EPIK_AMD_PERMDISP_PAIR_SLOTS 496u
#define EPIK_AMD_PERMDISP_MAX_PERMUTATIONS 999999u
#define EPIK_AMD_PERMDISP_MISSING 0xffffffffu
int epik_amd_cohort_permdisp_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, uint32_t num_columns,
                                    uint32_t num_permutations, uint64_t seed, int pairwise, void *d_out, void *d_stat,
                                    void *d_group_mean, void *d_z, void *stream);
int epik_amd_cohort_permdisp(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                             const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                             int pairwise, epik_amd_permdisp *out, double *stat, double *group_mean, double *z);
int epik_amd_cohort_permdisp_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                  const double *branch_length, const uint32_t *labels, uint32_t num_columns,
                                  uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permdisp *out, double *stat,
                                  double *group_mean, double *z);
int epik_amd_cohort_permdisp_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                    uint32_t metric, const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations,
                                    uint64_t seed, int pairwise, epik_amd_permdisp *out, double *stat, double *group_mean,
                                    double *z);
int epik_amd_cohort_permdisp_metric_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                         const double *branch_length, uint32_t metric, const uint32_t *labels,
                                         uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                         epik_amd_permdisp *out, double *stat, double *group_mean, double *z);
int epik_amd_cohort_permdisp_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                     uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                     epik_amd_permdisp *out, double *stat, double *group_mean, double *z);
int epik_amd_cohort_permdisp_strata_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, uint32_t num_columns,
                                           uint32_t num_permutations, uint64_t seed, int pairwise, void *d_out, void *d_stat,
                                           void *d_group_mean, void *d_z, void *stream, const uint32_t *strata);
int epik_amd_cohort_permdisp_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                    uint32_t metric, const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations,
                                    uint64_t seed, int pairwise, epik_amd_permdisp *out, double *stat, double *group_mean,
                                    double *z, const uint32_t *strata);
int epik_amd_cohort_permdisp_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                         const double *branch_length, uint32_t metric, const uint32_t *labels,
                                         uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                         epik_amd_permdisp *out, double *stat, double *group_mean, double *z,
                                         const uint32_t *strata);
int epik_amd_cohort_permdisp_strata_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                            uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                            epik_amd_permdisp *out, double *stat, double *group_mean, double *z,
                                            const uint32_t *strata);
typedef struct epik_amd_model_term {
    uint32_t df, columns; /* the accepted columns of the term and all of them; R and C for the whole model */
    uint64_t at_least;    /* #{p >= 1 : F(sigma_p) >= F(sigma_0)} */
    double ss, f, r2, p;
} epik_amd_model_term; /* 48 bytes */
typedef struct epik_amd_model_info {
    uint32_t used, terms, columns, rank; /* L, T, C, R */
    int64_t df_res;                      /* L - 1 - R */
    double ss_total, ss_res;
} epik_amd_model_info; /* 40 bytes */
#define EPIK_AMD_MODEL_MAX_TERMS 16u
#define EPIK_AMD_MODEL_MAX_COLUMNS 64u
#define EPIK_AMD_MODEL_MAX_GROUPS 32u
#define EPIK_AMD_MODEL_MAX_PERMUTATIONS 999999u
#define EPIK_AMD_MODEL_MISSING 0xffffffffu
int epik_amd_cohort_model_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *kind, const uint32_t *labels,
                                 const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed, void *d_out,
                                 void *d_info, void *d_stat, void *d_aliased, void *stream);
int epik_amd_cohort_model(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, const uint32_t *kind,
                          const uint32_t *labels, const double *values, uint32_t num_terms, uint32_t num_permutations,
                          uint64_t seed, epik_amd_model_term *out, epik_amd_model_info *info, double *stat, uint8_t *aliased);
int epik_amd_cohort_model_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                 const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t num_terms,
                                 uint32_t num_permutations, uint64_t seed, epik_amd_model_term *out, epik_amd_model_info *info,
                                 double *stat, uint8_t *aliased);
int epik_amd_cohort_model_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                               const double *branch_length, const uint32_t *kind, const uint32_t *labels, const double *values,
                               uint32_t num_terms, uint32_t num_permutations, uint64_t seed, epik_amd_model_term *out,
                               epik_amd_model_info *info, double *stat, uint8_t *aliased);
int epik_amd_cohort_model_metric_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                      const double *branch_length, uint32_t metric, const uint32_t *kind, const uint32_t *labels,
                                      const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                                      epik_amd_model_term *out, epik_amd_model_info *info, double *stat, uint8_t *aliased);
int epik_amd_cohort_model_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *kind,
                                  const uint32_t *labels, const double *values, uint32_t num_terms, uint32_t num_permutations,
                                  uint64_t seed, epik_amd_model_term *out, epik_amd_model_info *info, double *stat,
                                  uint8_t *aliased);
int epik_amd_cohort_model_strata_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *kind, const uint32_t *labels,
                                        const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                                        void *d_out, void *d_info, void *d_stat, void *d_aliased, void *stream,
                                        const uint32_t *strata);
int epik_amd_cohort_model_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                 const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t num_terms,
                                 uint32_t num_permutations, uint64_t seed, epik_amd_model_term *out, epik_amd_model_info *info,
                                 double *stat, uint8_t *aliased, const uint32_t *strata);
int epik_amd_cohort_model_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                      const double *branch_length, uint32_t metric, const uint32_t *kind, const uint32_t *labels,
                                      const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                                      epik_amd_model_term *out, epik_amd_model_info *info, double *stat, uint8_t *aliased,
                                      const uint32_t *strata);
int epik_amd_cohort_model_strata_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *kind,
                                         const uint32_t *labels, const double *values, uint32_t num_terms,
                                         uint32_t num_permutations, uint64_t seed, epik_amd_model_term *out,
                                         epik_amd_model_info *info, double *stat, uint8_t *aliased, const uint32_t *strata);
typedef struct epik_amd_edgemodel_family {
    double ss, r2, partial_r2, f, p, p_adj;
    uint64_t at_least, max_at_least; /* #{p >= 1 : phi(sigma_p) >= partial_r2}, #{p >= 1 : Mmax_p >= partial_r2} */
    int32_t sign;                    /* of s_c for a term with one accepted column; 0 otherwise */
    uint32_t pad;                    /* 0 */
} epik_amd_edgemodel_family; /* 72 bytes */
typedef struct epik_amd_edgemodel {
    epik_amd_edgemodel_family family[2]; /* mass, imbalance */
} epik_amd_edgemodel; /* 144 bytes */
typedef struct epik_amd_edgemodel_info {
    uint32_t used, terms, columns, rank; /* L, T, C, R: the model's */
    int64_t df_res;                      /* L - 1 - R */
    uint32_t df[16], term_columns[16];   /* the accepted columns of a term and all of them; 0 beyond T */
} epik_amd_edgemodel_info; /* 152 bytes */
#define EPIK_AMD_EDGEMODEL_FAMILIES 2u
int epik_amd_cohort_edgemodel_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind,
                                     const uint32_t *labels, const double *values, uint32_t num_terms, uint32_t num_permutations,
                                     uint64_t seed, void *d_out, void *d_info, void *d_stat, void *d_max, void *d_aliased,
                                     void *stream);
int epik_amd_cohort_edgemodel(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind, const uint32_t *labels,
                              const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                              epik_amd_edgemodel *out, epik_amd_edgemodel_info *info, double *stat, double *max, uint8_t *aliased);
int epik_amd_cohort_edgemodel_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                   const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t num_terms,
                                   uint32_t num_permutations, uint64_t seed, epik_amd_edgemodel *out,
                                   epik_amd_edgemodel_info *info, double *stat, double *max, uint8_t *aliased);
int epik_amd_cohort_edgemodel_strata_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind,
                                            const uint32_t *labels, const double *values, uint32_t num_terms,
                                            uint32_t num_permutations, uint64_t seed, void *d_out, void *d_info, void *d_stat,
                                            void *d_max, void *d_aliased, void *stream, const uint32_t *strata);
int epik_amd_cohort_edgemodel_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *kind,
                                     const uint32_t *labels, const double *values, uint32_t num_terms, uint32_t num_permutations,
                                     uint64_t seed, epik_amd_edgemodel *out, epik_amd_edgemodel_info *info, double *stat,
                                     double *max, uint8_t *aliased, const uint32_t *strata);
int epik_amd_cohort_edgemodel_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                          const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t num_terms,
                                          uint32_t num_permutations, uint64_t seed, epik_amd_edgemodel *out,
                                          epik_amd_edgemodel_info *info, double *stat, double *max, uint8_t *aliased,
                                          const uint32_t *strata);
int epik_amd_placer_cohort_reads(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                                 const uint32_t *weights, const uint32_t *samples, uint64_t n);
int epik_amd_placer_cohort_strands(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                                   const uint32_t *weights, const uint32_t *samples, uint64_t n, uint32_t mode,
                                   uint8_t *strand);
int epik_amd_placer_cohort_frames(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                                  const uint32_t *weights, const uint32_t *samples, uint64_t n, uint32_t mode, uint8_t *frame);
int epik_amd_placer_cohort_mates(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                                 const uint32_t *weights, const uint32_t *samples, uint64_t n_pairs, uint32_t mode,
                                 uint8_t *strand);

/*
 * Taxonomic assignment of reads and samples, computed on the device from the rows a placement wrote: the lowest taxon
 * that holds a given share of a read's placement mass, and per sample the reads assigned to and the mass placed in
 * every taxon.  No reference counterpart: the reference writes a jplace and leaves the question to a second tool.  One
 * rule; the kernel (taxa_place.hip), the host mirror (epik_amd/host/taxonomy.cpp) and the tests' numpy
 * are worded after it and must agree bit for bit.
 *
 * The taxonomy.  A text file, one line per reference leaf: leaf_label <TAB> taxopath, the taxopath A;B;C.  Blank lines
 *   and lines that begin with '#' are skipped; blanks around the label and around every path element are stripped; an
 *   empty element, or a line without a tab, is an error that names the line ("line <n>: ..."), and so is a leaf given
 *   twice (the second line).  The taxopath "-" is the empty path.  The taxa are the distinct non-empty prefixes of all
 *   taxopaths and a root, the empty path.  Ids are post-order over this trie, the children of a taxon in bytewise order
 *   of their names: the root is T - 1, taxon_parent[t] > t for t < T - 1 and taxon_parent[T - 1] =
 *   EPIK_AMD_TREE_NO_PARENT -- the conventions of epik_amd_tree, whose validation, first[] and lca serve the taxonomy
 *   unchanged, with branch lengths of zero.
 *   label[b], b < N.  Of a leaf branch: the taxon of the leaf's full taxopath (a tree leaf that the file does not give
 *   is an error that names the leaf, a label of the file that is no leaf one that names its line).  Of an inner branch:
 *   the taxonomy lca of the labels of its children, which is their longest common prefix.  A row on branch b counts for
 *   the taxon shared by everything below b.
 *
 * The record of read i.  q(), keep and nr = min(n_rows[i], keep) are the confidence rule's, and the first four tests
 *   come in its order:
 *     n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW    taxon = EPIK_AMD_TAXON_TOO_NARROW, the other fields 0
 *     n_rows[i] == 0                                  taxon = EPIK_AMD_TAXON_TOO_SHORT,  the other fields 0
 *     kmer_counts[i * keep] == 0                      taxon = EPIK_AMD_TAXON_NO_HIT,     the other fields 0
 *     a row j < nr with branch >= N                   taxon = EPIK_AMD_TAXON_BAD_ROW,    the other fields 0
 *   otherwise t_j = label[b_j] and S = the sum over j < nr of q(lwr_j), an exact integer (uint64; with LWRs in [0, 1]
 *   and keep <= 64 it is at most 2^36):
 *     S == 0                                          taxon = EPIK_AMD_TAXON_NO_MASS,    the other fields 0
 *   otherwise, with mass(c) = the sum of q(lwr_j) over j < nr with first[c] <= t_j <= c:
 *   taxon         the lowest taxon c with mass(c) * 2^30 >= tau_q * S, compared as exact integers (they fit 67 bits;
 *                 nothing wraps -- unlike the confidence rule).  tau_q lies in (2^29, 2^30], anything else is
 *                 EPIK_AMD_ERR_INVALID: with more than half of the mass required, two taxa that qualify share a row,
 *                 so one holds the other -- the qualifying taxa are a chain that ends in the root, which always
 *                 qualifies, and the lowest of them is the one of the smallest id.
 *   taxon_mass_q  mass(taxon), saturating at 2^32 - 1.
 *   first_taxon   t_0.
 *   total_q       S, saturating at 2^32 - 1.
 *   The rule reads slots past n_rows nowhere.  The record is a pure function of the read's rows, label[] and the
 *   taxonomy: the same bits whatever the grid, the chunks or the stream.
 *
 * The cells.  num_samples rows, one per sample (1 outside a cohort); a row is direct[T] | assigned[T] | the totals,
 *   uint64 that wrap.  Read i belongs to sample samples[i] (NULL: 0) and has weight w (uint32; NULL: 1; 0 adds nothing):
 *     TOO_NARROW   totals.too_narrow += w          TOO_SHORT   totals.too_short += w
 *     NO_HIT       totals.no_hit += w              NO_MASS     totals.no_mass += w
 *     BAD_ROW      totals.bad_reads += 1, and nothing else
 *     otherwise    totals.placed += w; assigned[taxon] += w; direct[t_j] += w * q(lwr_j) for every j < nr
 *   samples[i] >= num_samples adds 1 to bad_samples and touches no row (the record is written all the same).  Integer
 *   adds commute: the cells are the same bits whatever the order, the grouping, the pieces or the devices summed
 *   afterwards.  The cells of a clade are a difference of a prefix sum over [first[t], t].
 *
 * An epik_amd_taxonomy is an object of its own, created for a placer's device, num_branches and keep_at_most (the
 * placer may be destroyed before it) from taxon_parent[num_taxa], label[num_branches] and num_samples >= 1; all zero at
 * create() and after reset().  create() refuses with EPIK_AMD_ERR_INVALID an invalid taxonomy ("taxon <t>: ...", the
 * checks of epik_amd_tree_create worded for taxa), a label >= num_taxa ("branch <b>: ...") and a k-mer-space shard.
 *   add_device   asynchronous on `stream`, allocates nothing: the records of the n reads whose rows, n_rows and k-mer
 *                counts (required) a placement left in device memory into d_records[n] (NULL: none are written) and
 *                their adds into the cells; d_weights, d_samples: uint32 [n] or NULL.  n == 0 does nothing.  Adds of
 *                one object may run on several streams at once.
 *   read         synchronises the device, then copies out direct[S][T], assigned[S][T], totals[S] and bad_samples (each
 *                may be NULL); add_cells adds such arrays in (the objects of several devices summed into one); reset
 *                zeroes the cells.
 *   info         num_taxa, num_samples, num_branches, and whether add_device sums the current sample in LDS first
 *                (16 * num_taxa bytes beside the kernel's own; EPIK_AMD_PROFILE_LDS=0|1, read at create(), forces
 *                either: tests).
 *   taxa_reads / _strands / _frames / _mates: place / place_strands / place_frames / place_mates with every chunk's rows
 *                added to `taxonomy` on the device, item i with weights[i] into row samples[i] (HOST uint32 [n], or NULL: 1
 *                and row 0; both are uploaded once).  records [n] (HOST, or NULL: no record is computed), rows, n_rows and
 *                kmer_counts may be NULL, each by itself: that part stays on the device.  `profile` or `cohort` (not
 *                both; a cohort needs samples): the same rows are also added to it there.  Refused with
 *                EPIK_AMD_ERR_INVALID: tau_q out of range, an object created for another placer (device, num_branches or
 *                keep_at_most differ), a k-mer-space shard, nulls.  Synchronous.
 *   add_device takes raw device pointers and cannot know which placer wrote them: the caller answers for rows of the
 *   object's keep_at_most and num_branches.  A batch holds fewer than 2^32 reads (EPIK_AMD_ERR_INVALID otherwise).
 *   assign_host  the same rule with no device: records[n] (may be NULL) and the cells ADDED into direct[S][T],
 *                assigned[S][T], totals[S] and *bad_samples (all four, or none of them).
 */
#define EPIK_AMD_TAXON_TOO_NARROW 0xffffffffu
#define EPIK_AMD_TAXON_TOO_SHORT 0xfffffffeu
#define EPIK_AMD_TAXON_NO_HIT 0xfffffffdu
#define EPIK_AMD_TAXON_BAD_ROW 0xfffffffcu
#define EPIK_AMD_TAXON_NO_MASS 0xfffffffbu
typedef struct {
    uint32_t taxon;
    uint32_t taxon_mass_q;
    uint32_t first_taxon;
    uint32_t total_q;
} epik_amd_taxon_record; /* 16 bytes */
typedef struct {
    uint64_t placed;     /* weighted reads that were assigned a taxon */
    uint64_t no_hit;     /* ... whose rows are fabricated: none of their k-mers is in the database */
    uint64_t too_short;  /* ... shorter than k */
    uint64_t too_narrow; /* ... EPIK_AMD_ROWS_COUNTS_TOO_NARROW (device-pointer launches only) */
    uint64_t no_mass;    /* ... whose rows hold no mass at all */
    uint64_t bad_reads;  /* reads (not weighted) with a row whose branch is >= num_branches */
} epik_amd_taxa_totals;
typedef struct epik_amd_taxonomy epik_amd_taxonomy;
int epik_amd_taxonomy_create(const epik_amd_placer *p, const uint32_t *taxon_parent, uint32_t num_taxa,
                             const uint32_t *label, uint32_t num_samples, epik_amd_taxonomy **out);
void epik_amd_taxonomy_destroy(epik_amd_taxonomy *taxonomy);
int epik_amd_taxonomy_reset(epik_amd_taxonomy *taxonomy);
int epik_amd_taxonomy_info(const epik_amd_taxonomy *taxonomy, uint32_t *num_taxa, uint32_t *num_samples,
                           uint32_t *num_branches, uint32_t *lds_path);
int epik_amd_taxonomy_read(epik_amd_taxonomy *taxonomy, uint64_t *direct, uint64_t *assigned,
                           epik_amd_taxa_totals *totals, uint64_t *bad_samples);
int epik_amd_taxonomy_add_cells(epik_amd_taxonomy *taxonomy, const uint64_t *direct, const uint64_t *assigned,
                                const epik_amd_taxa_totals *totals);
int epik_amd_taxonomy_add_device(epik_amd_taxonomy *taxonomy, const void *d_rows, const void *d_n_rows,
                                 const void *d_kmer_counts, const void *d_weights, const void *d_samples, uint64_t n,
                                 uint32_t tau_q, void *d_records, void *stream);
int epik_amd_taxonomy_assign_host(const uint32_t *taxon_parent, uint32_t num_taxa, const uint32_t *label,
                                  uint32_t num_branches, uint32_t keep, const epik_amd_placement *rows,
                                  const uint32_t *n_rows, const uint32_t *kmer_counts, const uint32_t *weights,
                                  const uint32_t *samples, uint64_t n, uint32_t num_samples, uint32_t tau_q,
                                  epik_amd_taxon_record *records, uint64_t *direct, uint64_t *assigned,
                                  epik_amd_taxa_totals *totals, uint64_t *bad_samples);

int epik_amd_placer_taxa_reads(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                               epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                               epik_amd_taxonomy *taxonomy, uint32_t tau_q, epik_amd_taxon_record *records,
                               const uint32_t *weights, const uint32_t *samples, epik_amd_profile *profile,
                               epik_amd_cohort *cohort);
int epik_amd_placer_taxa_strands(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                 uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                 uint8_t *strand, epik_amd_taxonomy *taxonomy, uint32_t tau_q,
                                 epik_amd_taxon_record *records, const uint32_t *weights, const uint32_t *samples,
                                 epik_amd_profile *profile, epik_amd_cohort *cohort);
int epik_amd_placer_taxa_frames(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                uint8_t *frame, epik_amd_taxonomy *taxonomy, uint32_t tau_q,
                                epik_amd_taxon_record *records, const uint32_t *weights, const uint32_t *samples,
                                epik_amd_profile *profile, epik_amd_cohort *cohort);
int epik_amd_placer_taxa_mates(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n_pairs,
                               uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                               uint8_t *strand, epik_amd_taxonomy *taxonomy, uint32_t tau_q,
                               epik_amd_taxon_record *records, const uint32_t *weights, const uint32_t *samples,
                               epik_amd_profile *profile, epik_amd_cohort *cohort);

/*
 * Long sequences painted by windows.  No reference counterpart (SHERPAS, a sibling of the reference, does it with
 * phylo-k-mers on the CPU): a query longer than one evolutionary history -- a recombinant genome, a chimeric amplicon,
 * a contig -- is cut into windows, every window is placed by itself, called for the group of branches that holds its
 * mass, and the runs of windows that agree are reported with the places where the call changes.
 *
 * The windows of a read of L characters, window W and step S, k <= W < 2^31, 1 <= S <= W (epik_amd_window_span):
 *   L <= W   one window [0, L) -- for L = 0 too: such a window comes back with n_rows 0 like any read shorter than k;
 *   L >  W   nw = 1 + ceil((L - W) / S) windows; window w < nw - 1 is [w S, w S + W), the last one [L - W, L): the
 *            tail is always covered.
 *   win_offsets[n + 1] is the exclusive sum of nw over the batch: read i owns the windows win_offsets[i] ..
 *   win_offsets[i + 1] - 1 of every per-window array.  A read of more than EPIK_AMD_WINDOW_MAX_PER_READ windows is
 *   EPIK_AMD_ERR_INVALID in the host entry; to the device entry the caller answers for it.
 *
 * Placement.  Every window is a read of its own to the placement: rows [num_windows][keep], n_rows [num_windows],
 * k-mer counts [num_windows][keep] and a strand byte [num_windows] are those place_strands gives for the windows' bytes
 * with the same `mode`; with BOTH every window picks its own strand by that rule.  Amino-acid handles take FORWARD only
 * (the strand placement's own check refuses the rest); whole databases only.
 *   place_windows_device  asynchronous on `stream`, never allocates, count width as the caller chose it (the longest
 *       window is min(longest read, W)).  num_windows and window_bytes are the batch's totals as epik_amd_window_span
 *       gives them (window_bytes: the sum of the windows' lengths); the output buffers hold num_windows items and
 *       d_workspace at least window_workspace_bytes(n, num_windows, window_bytes, mode).  The kernels count and cut by
 *       themselves and clamp every write to those totals: totals that do not fit the batch give wrong windows, never a
 *       write outside.  d_kmer_counts, d_strand and d_win_offsets (uint64 [n + 1]) may be NULL.
 *   place_windows         synchronous, host buffers sized by the caller from epik_amd_window_span.  Chunks are cut on
 *       READ boundaries by a budget of windows and window bytes (EPIK_AMD_WINDOW_CHUNK_WINDOWS overrides the former:
 *       tests).  A read is never split across chunks in this version: one whose windows do not fit the device fails
 *       with the allocation's error (EPIK_AMD_ERR_HIP).  The count width is chosen for min(longest read, W): no window
 *       comes back EPIK_AMD_ROWS_COUNTS_TOO_NARROW.  kmer_counts, strand and win_offsets may be NULL.
 *
 * Painting.  group[b], b < N, is the group id of branch b or EPIK_AMD_WINDOW_NO_GROUP for a branch above the groups
 * (ids at or above EPIK_AMD_WINDOW_AMBIGUOUS are refused by the host entry).  q(), keep and nr = min(n_rows, keep) are
 * the taxa rule's; the record of window v, the tests in this order:
 *     n_rows[v] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW    call = EPIK_AMD_WINDOW_TOO_NARROW
 *     n_rows[v] == 0                                  call = EPIK_AMD_WINDOW_TOO_SHORT
 *     kmer_counts[v * keep] == 0                      call = EPIK_AMD_WINDOW_NO_HIT
 *     a row j < nr with branch >= N                   call = EPIK_AMD_WINDOW_BAD_ROW
 *     S = the sum over j < nr of q(lwr_j) is 0        call = EPIK_AMD_WINDOW_NO_MASS
 *   otherwise mass(g) = the sum of q(lwr_j) over j < nr with group[b_j] == g (NO_GROUP is in no mass: those rows count
 *   in S only) and call = the group g with mass(g) * 2^30 >= tau_q * S, compared as exact integers.  tau_q lies in
 *   (2^29, 2^30], anything else is EPIK_AMD_ERR_INVALID: at most one group then qualifies.  None does:
 *   call = EPIK_AMD_WINDOW_AMBIGUOUS.  A record with a status call has its other fields 0; else call_mass_q =
 *   mass(call) and total_q = S, both saturating at 2^32 - 1, and first_group = group[b_0].
 *   A segment of a read is a maximal run of consecutive windows with equal call; status calls count as values.  Its
 *   record: the call, its first window (counted inside the read), its number of windows, and the sums over its windows
 *   of the unsaturated mass(call) and S (both 0 for a status call).  Read i has n_segments[i] of them, written to the
 *   slots win_offsets[i] + s, s < n_segments[i]; slots beyond are left alone by the device entry and zeroed by the
 *   host entry.  Records and segments are a pure function of the rows: the same bits whatever the grid or the stream.
 *   windows_paint_device  asynchronous on `stream` of `device`, allocates nothing; all pointers are device memory,
 *       num_windows = win_offsets[n] as the caller knows it (windows beyond it are not looked at).
 *   windows_paint_host    the same rule with no device.
 *   paint_windows         place_windows with every chunk's windows painted on the device from the rows the placement
 *       left there: group[num_branches of the placer] (HOST) is uploaded once; records [num_windows], segments
 *       [num_windows] and n_segments [n] are host arrays.  rows, n_rows, kmer_counts, strand, win_offsets, records,
 *       segments and n_segments may be NULL, each by itself: that part stays on the device.  Synchronous.
 */
#define EPIK_AMD_WINDOW_MAX_PER_READ (1u << 24)
#define EPIK_AMD_WINDOW_NO_GROUP 0xffffffffu
#define EPIK_AMD_WINDOW_TOO_NARROW 0xffffffffu
#define EPIK_AMD_WINDOW_TOO_SHORT 0xfffffffeu
#define EPIK_AMD_WINDOW_NO_HIT 0xfffffffdu
#define EPIK_AMD_WINDOW_BAD_ROW 0xfffffffcu
#define EPIK_AMD_WINDOW_NO_MASS 0xfffffffbu
#define EPIK_AMD_WINDOW_AMBIGUOUS 0xfffffffau
typedef struct {
    uint32_t call;
    uint32_t call_mass_q;
    uint32_t first_group;
    uint32_t total_q;
} epik_amd_window_record; /* 16 bytes */
typedef struct {
    uint32_t call;
    uint32_t first_window;
    uint32_t num_windows;
    uint32_t reserved; /* 0 */
    uint64_t call_mass;
    uint64_t total;
} epik_amd_window_segment; /* 32 bytes */

/* The number of windows of a read of `len` characters (0: window or step out of range); for w below it *begin and
 * *end (either may be NULL) get window w, 0-based half-open in the read.  Defined here, so that a caller sizes its buffers
 * without a call into the library and a kernel can use it; libepik_amd exports it as well (a binding without a C compiler). */
#if defined(__HIP__)
#define EPIK_AMD_INLINE inline __attribute__((host)) __attribute__((device))
#elif defined(__cplusplus)
#define EPIK_AMD_INLINE inline
#else
#define EPIK_AMD_INLINE static inline
#endif
EPIK_AMD_INLINE uint64_t epik_amd_window_span(uint64_t len, uint32_t window, uint32_t step, uint64_t w,
                                              uint64_t *begin, uint64_t *end)
{
    if (window == 0 || window >= 0x80000000u || step == 0 || step > window) return 0;
    const uint64_t nw = len <= window ? 1 : 1 + (len - window + step - 1) / step;
    if (w < nw) {
        const uint64_t b = len <= window ? 0 : w + 1 < nw ? w * step : len - window;
        if (begin) *begin = b;
        if (end) *end = len <= window ? len : b + window;
    }
    return nw;
}

int epik_amd_placer_window_workspace_bytes(const epik_amd_placer *p, uint64_t n, uint64_t num_windows,
                                           uint64_t window_bytes, uint32_t mode, uint64_t *bytes);
int epik_amd_placer_place_windows_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n,
                                         uint32_t window, uint32_t step, uint32_t mode, uint64_t num_windows,
                                         uint64_t window_bytes, void *d_workspace, uint64_t workspace_bytes,
                                         void *d_rows, void *d_n_rows, void *d_kmer_counts, void *d_strand,
                                         void *d_win_offsets, void *stream);
int epik_amd_placer_place_windows(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                  uint32_t window, uint32_t step, uint32_t mode, epik_amd_placement *rows,
                                  uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *strand, uint64_t *win_offsets);
int epik_amd_placer_paint_windows(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                  uint32_t window, uint32_t step, uint32_t mode, const uint32_t *group, uint32_t tau_q,
                                  epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *strand,
                                  uint64_t *win_offsets, epik_amd_window_record *records,
                                  epik_amd_window_segment *segments, uint32_t *n_segments);
int epik_amd_windows_paint_device(int device, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                                  const void *d_win_offsets, uint64_t n, uint64_t num_windows, uint32_t keep,
                                  const void *d_group, uint32_t num_branches, uint32_t tau_q, void *d_records,
                                  void *d_segments, void *d_n_segments, void *stream);
int epik_amd_windows_paint_host(const epik_amd_placement *rows, const uint32_t *n_rows, const uint32_t *kmer_counts,
                                const uint64_t *win_offsets, uint64_t n, uint32_t keep, const uint32_t *group,
                                uint32_t num_branches, uint32_t tau_q, epik_amd_window_record *records,
                                epik_amd_window_segment *segments, uint32_t *n_segments);

/*
 * Building a phylo-k-mer database from ancestral posteriors.  The reference's world does this in a second product
 * (IPK, after RAPPAS: PAPERS.md) on CPU threads; the rule below is this project's own, worded so that the device, the
 * host mirror and a numpy restatement give the same bytes.
 *
 * Inputs.  sigma is 4 or 20; k lies in [2, 15] for sigma = 4 and in [2, 7] for sigma = 20 (keys stay inside uint32);
 * num_branches is N >= 1; log_thr is a float32, at most 0 and no NaN (the caller passes log10f((omega / sigma)^k) as
 * the placement computes it).  Ghost nodes arrive in chunks: logp float32 [G][L][sigma], log10 of the posterior of
 * every state at every site (every value at most 0, -inf for p = 0; NaN and values above 0 are refused), and branch_of
 * uint32 [G], every value below N, repeats and any order allowed.  L >= k is the same for every chunk of one build.
 * The logarithm is the caller's (log10f on the host); the device never evaluates one.
 *
 * The rule.  For ghost node g, window start w in [0, L - k] and letters c_0 .. c_{k-1}:
 *     s = ((((+0.0f + logp[g][w][c_0]) + logp[g][w+1][c_1]) + ...) + logp[g][w+k-1][c_{k-1}])
 * in float32, left to right, every addition rounded to nearest (no contraction).  The k-mer survives iff
 * s >= log_thr (the loader's comparison), and its key is the sum of c_j sigma^(k-1-j): first letter most significant.
 * The value of (key, b) is the maximum of s over every surviving (g, w) with branch_of[g] = b.
 *   Zeros.  The chain starts from +0.0f, and in round-to-nearest (+0) + (-0) = +0 and x + y of two values <= 0 is
 *   -0 only when both are -0: a sum that starts from +0.0 never produces -0.0, even over logp values given as -0.0.
 *   +0.0 and -0.0 therefore never both occur as a score, and "maximum" needs no rule for them.
 *   Pruning cannot change the result.  Rounded addition is monotone in each operand, so the left-to-right sum of a
 *   prefix completed with the best remaining letter of every position is the maximum over its completions, and a
 *   prefix whose completed sum is below log_thr has no survivor.  The kernels and the host mirror cut a prefix of
 *   depth d when fl(s_d + R_d) < log_thr (1 + 16 k 2^-24) (rounded away from 0), R_d the float32 right-to-left sum
 *   of the best remaining letters: both fl(s_d + R_d) and the completed sum are sums of at most k + 1 values of one
 *   sign and lie within (1 +- 2^-24)^(k+1) of the exact sum, so the cut is never taken for a prefix with a survivor;
 *   what it lets through is tested exactly at depth k.
 *   Chunking cannot change the result either: maximum is associative and commutative and the survivors of a ghost
 *   node depend on nothing but that node, so any split of the ghost nodes into chunks, and any split of a chunk
 *   inside the library, gives the same bytes.
 *
 * The result has the sparse CSR form of the placer's descriptor: keys uint32 [K] ascending, one per key with at least
 * one value; offsets uint64 [K + 1]; values [E] {branch, score}, branch ascending within a key.  K = 0 is valid.
 *
 *   builder_create   a builder on `device`; workspace_bytes is what the enumeration of one chunk may use on the
 *       device (its per-window counts and its (key, branch, score) tuples at 40 bytes each; 0: 1 GiB).  A chunk
 *       whose tuples do not fit is split by ghost nodes inside `add`, as often as needed; only a single ghost node
 *       that does not fit is EPIK_AMD_ERR_INVALID (the message says how many bytes it needs; the ghost nodes of the
 *       chunk before it have been added by then, the others have not).  Beside the workspace
 *       the builder holds its running store (12 bytes an entry, sorted and deduplicated; twice while a chunk is
 *       merged in) and the scratch of hipCUB's scans and sorts.
 *   builder_add          logp and branch_of are HOST arrays; synchronous.
 *   builder_add_device   the same with DEVICE arrays on the builder's device; synchronous as well (the counts of a
 *       chunk size its tuples).
 *       Both refuse, with EPIK_AMD_ERR_INVALID and nothing added to the store: a NaN or a value above 0 (the message
 *       names the first one's ghost node, site and state), branch_of[g] >= N (names g), L < k, L other than the
 *       first chunk's.  G = 0 is a valid no-op.
 *   builder_finish   the sizes of the result; *num_splits (may be NULL) gets how many times `add` has split a chunk
 *       so far.  More chunks may be added afterwards; finish then has to be called again before copy.
 *   builder_copy     the result into HOST arrays of those sizes.
 *   build_host       the same rule in plain C++ on `num_threads` threads (0: one), no device: pruned depth-first
 *       enumeration and a std::sort merge.  *result is a finished builder that finish, copy and destroy take.
 */
typedef struct epik_amd_builder epik_amd_builder;
int epik_amd_builder_create(int device, uint32_t sigma, uint32_t k, uint32_t num_branches, float log_thr,
                            uint64_t workspace_bytes, epik_amd_builder **builder);
int epik_amd_builder_add(epik_amd_builder *builder, const float *logp, const uint32_t *branch_of, uint64_t G, uint64_t L);
int epik_amd_builder_add_device(epik_amd_builder *builder, const void *d_logp, const void *d_branch_of, uint64_t G,
                                uint64_t L);
int epik_amd_builder_finish(epik_amd_builder *builder, uint64_t *num_keys, uint64_t *num_entries, uint64_t *num_splits);
int epik_amd_builder_copy(epik_amd_builder *builder, uint32_t *keys, uint64_t *offsets, epik_amd_pkdb_value *values);
void epik_amd_builder_destroy(epik_amd_builder *builder);
int epik_amd_build_host(uint32_t sigma, uint32_t k, uint32_t num_branches, float log_thr, const float *logp,
                        const uint32_t *branch_of, uint64_t G, uint64_t L, uint32_t num_threads,
                        epik_amd_builder **result);

/*
 * Reconstructing ancestral posteriors: the marginal posterior of every state at every site of the ghost nodes of a
 * reference tree, by Felsenstein's pruning algorithm -- what the builder above starts from.  Model
 * parameters are given, never optimised.  The rule below is this project's own, worded so that the device, the host
 * mirror and a numpy restatement give the same bytes.
 *
 * Inputs.  The reference tree as parent int32 [N] in the numbering of the drivers: post-order (parent[v] > v), the
 * root N - 1 with parent -1, every inner node with exactly two children, N >= 3.  sigma is 4 or 20; C in [1, 8] rate
 * categories with weights w double [C]; frequencies pi double [sigma]; three tables of transition matrices, double
 * [N - 1][C][sigma][sigma] each, row = the state at the upper end: p_full of the whole branch above node b, p_half of
 * half that branch, p_pend of the pendant length of the ghost nodes of b.  Every weight and frequency is finite and
 * at least 0, every matrix entry lies in [0, 2].  The device evaluates no exp: the tables are an input.
 * masks uint32 [leaves][L]: per leaf (in the order of node ids) and site the set of states the character may stand
 * for, bit y for state y; a mask without any of the sigma low bits (a gap, an invalid character) counts as all states.
 *
 * Arithmetic.  Everything is IEEE double, rounded to nearest, no contraction of multiply and add, in the order given.
 * "sum over y" means ((t_0 + t_1) + t_2) + ... in state order starting from the first term.
 *   Down pass, post-order.  For a node u, site s, category c: F(u)[x] = sum over y of P_u,c[x][y] * D_u[s][c][y], P_u
 *   from p_full; for a leaf D_u[y] is 1.0 or 0.0 by its mask.  For an inner node v with children l, r:
 *   D_v[s][c][x] = F(l)[x] * F(r)[x].
 *   Up pass, pre-order.  U_v is the partial at parent(v) of everything outside v's subtree.  For a child of the root
 *   U_v[x] = F(sibling)[x]; otherwise U_v[x] = F(sibling)[x] * G(p)[x], p the parent and
 *   G(p)[x] = sum over z of P_p,c[x][z] * U_p[s][c][z].
 *   Scaling.  After each D_v and each U_v: m = the maximum of the site's C sigma entries; if m > 0,
 *   with m = f 2^e, f in [0.5, 1) (frexp), every entry becomes ldexp(entry, -e).  The exponent is not kept: a factor
 *   per site cancels in a posterior.  (No entry exceeds 1600 before scaling, so nothing overflows; scaling is exact
 *   unless an entry falls below the normal range, where ldexp rounds to nearest even on all three implementations.)
 *   Midpoint M_b of branch b < N - 1, with h = p_half[b][c]:
 *       A_c[x] = (sum over y of h[x][y] * D_b[y]) * (sum over z of h[x][z] * U_b[z]),   T_c[x] = pi[x] * A_c[x],
 *       n[x] = sum over c, in order from the first term, of w_c * T_c[x],   Z = sum over x of n[x],   p[x] = n[x] / Z.
 *   Pendant node P_b, with q = p_pend[b][c]: B_c[y] = sum over x of T_c[x] * q[x][y]; n[y] = sum over c of w_c * B_c[y];
 *   Z and p as above.  The two ghost leaves below P_b are all gaps and contribute factors of 1: the extended tree
 *   (epik_amd/dbbuild.py: extended_tree) is never materialised.
 *   Output.  p is rounded once to float32.  A row (ghost node, site) whose Z is 0 or not finite is all zeros, and
 *   *dead_sites counts those rows.  post is float32 [G][L][sigma] and branch_of uint32 [G]: ghosts =
 *   EPIK_AMD_GHOSTS_INNER gives G = N - 1 midpoints in branch order, _OUTER the N - 1 pendant nodes, _BOTH the
 *   midpoints followed by the pendant nodes (G = 2 (N - 1)).
 *   Sites are independent: the handle works through the alignment in chunks of sites, and a chunk cannot change a bit.
 *
 *   ancestral_create   a handle on `device` that holds the tree's tables and a workspace of workspace_bytes
 *       (0: 4 GiB) for the partials [inner nodes + N - 1][sites of a chunk][C][sigma] doubles, the masks and the
 *       posteriors of a chunk; a workspace that does not hold one site is EPIK_AMD_ERR_INVALID (the message says how
 *       many bytes a site needs).  The kernels take EPIK_AMD_ANCESTRAL_TILE_SITES sites a workgroup.
 *   ancestral_posteriors          masks HOST; post and branch_of HOST arrays; synchronous.
 *   ancestral_posteriors_device   masks HOST; d_post and d_branch_of DEVICE arrays on the handle's device (what
 *       epik_amd_builder_add_device takes once the logarithm has been taken); synchronous.
 *   ancestral_host     the same rule in plain C++ on `num_threads` threads (0: one) over the sites, no device.
 *   model_pmatrices    P(t) for every t of times[n], double [n][sigma][sigma]: the reversible model of the
 *       exchangeabilities (upper triangle row by row, sigma (sigma - 1) / 2 values) and frequencies pi (all above 0),
 *       Q normalised to one expected substitution per unit time, through sqrt(pi) symmetrisation and a Jacobi
 *       eigendecomposition; t = 0 gives the identity exactly.  Host only, not under the bit-for-bit rule.
 *   model_gamma_rates  the K <= 8 category means of a gamma distribution with shape = rate = alpha (Yang 1994), mean 1.
 */
#define EPIK_AMD_GHOSTS_INNER 0u
#define EPIK_AMD_GHOSTS_OUTER 1u
#define EPIK_AMD_GHOSTS_BOTH 2u
#define EPIK_AMD_ANCESTRAL_TILE_SITES 64u
typedef struct epik_amd_ancestral epik_amd_ancestral;
typedef struct epik_amd_ancestral_desc {
    uint32_t num_nodes;      /* N */
    uint32_t sigma;          /* 4 or 20 */
    uint32_t num_categories; /* C */
    uint32_t reserved;       /* 0 */
    const int32_t *parent;   /* [N] */
    const double *weights;   /* [C] */
    const double *pi;        /* [sigma] */
    const double *p_full;    /* [N - 1][C][sigma][sigma] */
    const double *p_half;
    const double *p_pend;
} epik_amd_ancestral_desc;
int epik_amd_ancestral_create(int device, const epik_amd_ancestral_desc *desc, uint64_t workspace_bytes,
                              epik_amd_ancestral **handle);
int epik_amd_ancestral_posteriors(epik_amd_ancestral *handle, const uint32_t *masks, uint64_t L, uint32_t ghosts,
                                  float *post, uint32_t *branch_of, uint64_t *dead_sites);
int epik_amd_ancestral_posteriors_device(epik_amd_ancestral *handle, const uint32_t *masks, uint64_t L, uint32_t ghosts,
                                         void *d_post, void *d_branch_of, uint64_t *dead_sites);
void epik_amd_ancestral_destroy(epik_amd_ancestral *handle);
int epik_amd_ancestral_host(const epik_amd_ancestral_desc *desc, const uint32_t *masks, uint64_t L, uint32_t ghosts,
                            uint32_t num_threads, float *post, uint32_t *branch_of, uint64_t *dead_sites);
int epik_amd_model_pmatrices(uint32_t sigma, const double *exchange, const double *pi, const double *times, uint64_t n,
                             double *out);
int epik_amd_model_gamma_rates(double alpha, uint32_t num_categories, double *rates);

/*
 * Ranking phylo-k-mers by informativeness: the order in which a database file stores its k-mers, which --mu and
 * --max-ram cut a prefix of.  The rule below is this project's own reading of "informative k-mers" (EPIK;
 * neither i2l nor IPK is available, so it is not IPK's formula: DESIGN.md, assumption register), worded so that the
 * device, the host mirror and a numpy restatement give the same bytes.
 *
 * Inputs.  A database in the sparse CSR form that builder_copy returns: keys uint32 [K] ascending, offsets uint64
 * [K + 1], values {branch, score}, branch ascending within a list, score a float32 log10 (at most 0, -inf allowed, no
 * NaN); N = num_branches >= 1; log_thr a float32, at most 0 (-inf allowed); a filter id; a uint64 seed.
 * Outputs.  value double [K], smaller = more informative, and order uint32 [K]: the permutation of 0 .. K - 1 sorted by
 * (value ascending, key ascending), -0.0 counted as +0.0 (value[] holds +0.0 then).  A value is never a NaN (below).
 *
 * Arithmetic.  IEEE double, rounded to nearest, no contraction of multiply and add, every parenthesis as written.
 *   LOG2_10 = 3.321928094887362, LN2 = 0.6931471805599453, TWO_OVER_LN2 = 2.8853900817779268,
 *   SQRT_HALF = 0.7071067811865476 (the doubles nearest to those constants).
 *   ek_exp2(x), x <= 1023:  +0.0 if x < -1022 (so -inf gives +0.0 and no result is subnormal); else n = rint(x) (ties to
 *     even), r = x - n (exact), y = r * LN2, q = c_13, then q = q * y + c_j for j = 12 .. 0 with c_j the double nearest
 *     to 1 / j!, and the result is ldexp(q, n) (exact: q lies in [0.70, 1.42] and x >= -1022 puts n = -1022 with r >= 0).
 *   ek_log2(z), z > 0 finite:  z = m 2^e, m in [0.5, 1) (frexp); if m < SQRT_HALF then m = m * 2 and e = e - 1;
 *     t = (m - 1.0) / (m + 1.0), u = t * t, q = d_11, then q = q * u + d_j for j = 10 .. 0 with d_j the double nearest to
 *     1 / (2 j + 1), and the result is (double)e + (t * q) * TWO_OVER_LN2.  (ek_log2(0) = -inf, ek_log2(+inf) = +inf and
 *     a NaN below 0: the rule never gets there.)
 *   The literal coefficients stand in epik_amd/host/filter.hpp, which the kernels and the host mirror both compile.
 *
 * EPIK_AMD_FILTER_MIF0: the conditional entropy H(B | w), in bits, of the branch given the k-mer, a branch without an
 * entry standing at the threshold probability.  For a list (b_i, s_i), i = 0 .. n - 1:
 *     x_i = (double)s_i * LOG2_10,   p_i = ek_exp2(x_i),   q_i = +0.0 if p_i == 0.0, else p_i * x_i
 *     A = SUM p_i,   B = SUM q_i                                               (SUM: below)
 *     x_t = (double)log_thr * LOG2_10,   t = ek_exp2(x_t),   M = (double)(N - n) (0.0 if n >= N)
 *     R = M * t,   C = +0.0 if R == 0.0, else R * x_t,   Z = A + R
 *     value = +inf if Z == 0.0, else ek_log2(Z) - ((B + C) / Z)
 *   SUM over the entries does not depend on the grid or on how many lanes serve a key: 64 interleaved chains, entry i
 *   to chain i mod 64, each chain ((+0.0 + u_c) + u_{c+64}) + ... in ascending i, and the 64 chain sums combined by the
 *   butterfly a[c] = a[c] + a[c + h] for c < h, for h = 32, 16, 8, 4, 2, 1; SUM is a[0].  Addition is commutative, so a
 *   butterfly of lane exchanges (a[c] + a[c xor h] in every lane) gives the same bits.  Every p_i is >= +0.0 and every
 *   q_i <= 0, a chain starts from +0.0, and x + (+0.0) is x for every x but -0.0, which it turns into +0.0: no chain
 *   holds -0.0, the empty chains hold +0.0, and adding them changes nothing -- a list of n <= 64 entries may be summed
 *   in closed form, n <= 4: ((+0.0 + u_0) + (+0.0 + u_2)) + ((+0.0 + u_1) + (+0.0 + u_3)) with +0.0 for an absent entry.
 *   No NaN.  s_i = -inf or p_i = 0 contributes +0.0 to both sums (0 * -inf is never formed); log_thr = -inf gives
 *   t = 0, R = 0 and C = +0.0; every p_i that is not 0 is at least 2^-1022 and at most 1, so A, B, R and C are finite,
 *   Z is 0 or a normal number, and (B + C) / Z is finite (|x| <= 1022, so |B + C| <= 1022 Z).  Z == 0 (every entry at
 *   p = 0 and t = 0) gives +inf: such a key is ranked last.  n = N gives M = 0; N = 1 with its one entry at s = 0 gives
 *   ek_log2(1) - 0 / 1 = 0.  An empty list (builder_copy has none) follows the same formulas with A = B = +0.0.
 * EPIK_AMD_FILTER_BEST: value = -(double)max_i s_i (+inf for an empty list): the order dbfile.informativeness_order
 *   has always written.
 * EPIK_AMD_FILTER_RANDOM: in uint64 arithmetic mod 2^64 (the splitmix64 finaliser, as the permutation tests' key),
 *     z = seed + (uint64)key * 0x9E3779B97F4A7C15,  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9,
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB,  z = z ^ z >> 31,   value = (double)(z >> 11)   (exact: 53 bits).
 *   The mix is a bijection; two keys whose z differ only in the low 11 bits tie and are ordered by key.
 * Order.  value with -0.0 folded into +0.0 has the monotone image  u = bits ^ 0xFFFF.. if the sign bit is set, else
 * bits | 2^63; order is the stable sort of 0 .. K - 1 by u.
 *
 *   filter_rank_device  keys, offsets, values, value and order are DEVICE arrays on `device`; the work is enqueued on
 *       `stream` and the call returns after it has finished (the checks' findings and the bits in use of the images are
 *       read back; the sort's scratch, 20 bytes a key and hipCUB's own, is allocated once per call).  K < 2^31.
 *   filter_rank         the same with HOST arrays: uploaded, ranked on `device`, copied back.
 *   builder_rank        after builder_finish: a device builder's own device arrays, nothing uploaded; the finished
 *       result of epik_amd_build_host runs the host mirror on one thread.  value and order are HOST arrays [num_keys].
 *       The builder keeps the scratch of the call (32 bytes a key and hipCUB's own) until it is destroyed.
 *   filter_rank_host    the same rule in plain C++ on `num_threads` threads (0: one), no device.
 *   filter_math_host    exp2_out[i] = ek_exp2(x[i]) and log2_out[i] = ek_log2(x[i]) (either may be NULL): tests.
 * All refuse with EPIK_AMD_ERR_INVALID and a message that names the first offender: an unknown filter; offsets that
 * are not ascending (offsets[k + 1] below offsets[k] or above offsets[K]); a score that is a NaN or above 0; a branch
 * that is not below N -- in that order when several apply.  K = 0 is valid and touches no array.
 */
#define EPIK_AMD_FILTER_BEST 0u
#define EPIK_AMD_FILTER_MIF0 1u
#define EPIK_AMD_FILTER_RANDOM 2u
int epik_amd_filter_rank_device(int device, uint32_t num_branches, float log_thr, const void *d_keys, const void *d_offsets,
                                const void *d_values, uint64_t K, uint32_t filter, uint64_t seed, void *d_value,
                                void *d_order, void *stream);
int epik_amd_filter_rank(int device, uint32_t num_branches, float log_thr, const uint32_t *keys, const uint64_t *offsets,
                         const epik_amd_pkdb_value *values, uint64_t K, uint32_t filter, uint64_t seed, double *value,
                         uint32_t *order);
int epik_amd_builder_rank(epik_amd_builder *builder, uint32_t filter, uint64_t seed, double *value, uint32_t *order);
int epik_amd_filter_rank_host(uint32_t num_branches, float log_thr, const uint32_t *keys, const uint64_t *offsets,
                              const epik_amd_pkdb_value *values, uint64_t K, uint32_t filter, uint64_t seed,
                              uint32_t num_threads, double *value, uint32_t *order);
int epik_amd_filter_math_host(const double *x, uint64_t n, double *exp2_out, double *log2_out);

/* Which kernels the last launch of this handle ran (reports; a large-tree handle falls back from the three-kernel
 * placement to the one-kernel one when the device has no room for the scratch of a launch). */
#define EPIK_AMD_PATH_WAVE 0u            /* place_reads_kernel: one wavefront per read */
#define EPIK_AMD_PATH_TEAM_ONE_KERNEL 1u /* team_place_kernel: one workgroup per read */
#define EPIK_AMD_PATH_TEAM_STREAMED 2u   /* team_front_kernel + team_stream_kernel + team_merge_kernel (+ the other for the rest) */
int epik_amd_placer_last_path(const epik_amd_placer *p, uint32_t *path);
/* What the streaming kernel of a large-tree placer is, with the handle's current count width (diagnostics, tests):
 * *wide = 1: the build for slices so large that LDS keeps a CU to twelve waves, which holds the slice epilogue over
 * the touched quads; *sparse_quads = how many touched quads (4 rows each) an item may have to take that epilogue
 * (0: never).  Both 0 for a placer of the one-wavefront kernel. */
int epik_amd_placer_stream_build(const epik_amd_placer *p, uint32_t *wide, uint32_t *sparse_quads);

/* Gives back what the handle's launches have grown and kept: the scratch of large-tree launches (descriptor pool,
 * headers, slice results: up to ~1 GB after batches of a million reads), the staging buffers of the host entry
 * points, the buffers of place_sharded.  The database stays; the next launch allocates again what it needs.
 * Synchronises the handle's device. */
int epik_amd_placer_release_scratch(epik_amd_placer *p);

/* Launch geometry actually used (for reports): waves per workgroup (one read per wave with the
 * one-wavefront kernel, one slice of a read per wave on large trees), workgroups of the last launch,
 * dynamic LDS bytes per workgroup. */
int epik_amd_placer_launch_info(const epik_amd_placer *p, uint32_t *waves_per_block,
                                uint32_t *blocks, uint32_t *lds_bytes);

/* Times the last place_device launch on its own stream with HIP events recorded
 * around the kernel inside the library (milliseconds; <0 if none was recorded).
 * Event recording is enabled with epik_amd_placer_set_timing(p, 1). */
int epik_amd_placer_set_timing(epik_amd_placer *p, int enabled);
int epik_amd_placer_last_kernel_ms(epik_amd_placer *p, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif
