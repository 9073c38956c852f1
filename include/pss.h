/*
 * pss.h -- C ABI of libpss.so, the MI355X (gfx950) engine behind the
 * pysubstringsearch Writer/Reader API.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, returns an
 * int status (0 = ok, negative = error, see PSS_E*) and never throws or aborts.
 * Each declaration cites the reference interface (file:line under the
 * upstream tree, Intsights/PySubstringSearch v0.7.1) it replaces.  The
 * reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Handles are not thread-safe: one thread per handle at a time (the reference's
 * pyclass methods take `&mut self`, src/lib.rs:67,88,105,126,201).
 *
 * There is no CPU fallback: every compute entry point fails with PSS_EDEVICE
 * when no HIP device is usable.
 */
#ifndef PSS_H
#define PSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSS_OK 0
#define PSS_EINVAL (-1)   /* bad arguments            (libsais.c:6599-6602 returns -1) */
#define PSS_ENOMEM (-2)   /* host/device allocation   (libsais.c:6505-6507 returns -2) */
#define PSS_EIO (-3)      /* I/O error, errno is set  (io::Error -> OSError, src/lib.rs:55,71,112-118) */
#define PSS_ETOOBIG (-4)  /* "entry is too big"       (src/lib.rs:92-94 -> ValueError) */
#define PSS_EDEVICE (-5)  /* HIP runtime error / no device */
#define PSS_EFORMAT (-6)  /* malformed or truncated .idx (UnexpectedEof in src/lib.rs:175-179) */

typedef struct pss_writer pss_writer;
typedef struct pss_reader pss_reader;
typedef struct pss_result pss_result;

/* ---- library ---------------------------------------------------------- */

/* Number of visible HIP devices (0 when none / runtime unusable). */
int pss_device_count(void);

/* The devices a handle opened with device == -1 uses -- what the reference-shaped call (`Reader(path)`, `Writer(path)`,
 * no device argument) gets; the reference fans out over every core of the machine without being asked (rayon's global
 * pool, src/lib.rs:205-207):
 *   PSS_DEVICES=all | 0,1,...   every visible device / the listed ordinals (one may be listed more than once);
 *   else (unset, or set to nothing) PSS_DEVICE=k, LOCAL_RANK=k, SLURM_LOCALID=k, OMPI_COMM_WORLD_LOCAL_RANK=k or
 *        MV2_COMM_WORLD_LOCAL_RANK=k (a launcher runs one process per GPU): device k mod count;
 *   else every visible device.
 * Writes at most cap ordinals to out and returns how many (>= 1); -1 (message in pss_last_error) when PSS_DEVICES is set
 * to something that is neither 'all' nor a list of ordinals below the device count -- handles opened without a device then
 * fail with PSS_EINVAL instead of spreading over every GPU (round 5: it used to count as unset). */
int32_t pss_default_devices(int32_t *out, int32_t cap);

/* Copies the calling thread's last error message into buf (NUL-terminated,
 * truncated to cap); returns the untruncated length. */
size_t pss_last_error(char *buf, size_t cap);

/* Test hook: re-reads the PSS_* environment switches of the search path, which the library reads
 * once (when it first needs them) rather than on every call. */
int pss_reload_env(void);

/* Frees the grow-only HBM workspace of every device (the builder keeps ~45 n
 * bytes around for reuse; resident Reader chunks are not touched). */
int pss_release_workspace(void);

/* HBM (bytes) the grow-only workspaces of `device` hold right now: the suffix-array builder's buffers (~45 n bytes after a
 * build of an n-byte chunk, more for natural text: DESIGN.md 3), its helper line's, and the scratch of the search path.
 * Resident indexes are not counted (pss_reader_residency).  A Writer that shares a GPU with a resident Reader can see
 * what one chunk in flight costs and give it back (pss_release_workspace).  No reference counterpart. */
uint64_t pss_workspace_bytes(int32_t device);

/* The environment switches the library reads (csrc/knobs.h: one registry, every read goes through it): how many there
 * are, and for switch i its name, what an unset switch means, the values a fuzzer may set (separated by '|'; empty: not
 * drawn) and what it does.  The strings are static.  None of the switches changes a result.  No reference counterpart. */
int32_t pss_knob_count(void);
int pss_knob_info(int32_t i, const char **name, const char **dflt, const char **fuzz, const char **what);

/* sizeof(pss_sa_stats) / sizeof(pss_search_stats) as the library was built: a binding that declares the structs itself
 * (ctypes, cgo, JNI) compares them with its own before the first call that fills one. */
uint64_t pss_sa_stats_size(void);
uint64_t pss_search_stats_size(void);

/* ---- suffix-array builder seam ----------------------------------------- */

/* Per-build statistics (filled when `stats` is non-NULL). */
typedef struct pss_sa_stats {
    uint32_t sigma;            /* distinct byte values in the text */
    uint32_t code_bits;        /* bits per recoded symbol (b) */
    uint32_t key_chars;        /* symbols packed into the initial 64-bit key (h0) */
    uint32_t initial_passes;   /* radix passes of the initial key sort */
    uint32_t rounds;           /* prefix-doubling rounds executed after it */
    uint32_t round_passes;     /* radix passes summed over all rounds */
    uint64_t sum_active;       /* sum over rounds of suffixes still unresolved */
    uint64_t sort_elems;       /* sum over every radix pass of elements moved */
    double ms_total;           /* device time of the whole build (HIP events) */
    double ms_sort;            /* device time inside radix passes (profile mode only) */
    uint64_t sort_launches;    /* radix-pass (scatter kernel) launches */
    /* profile mode: rs_scatter_kernel<false>, the generic (u64 key, u32 value) pass of the rounds
     * and of the sizing sample (reads 8 B key + 4 B value, writes the same: 24 B per element) */
    double ms_pairs;           /* summed duration of its launches */
    uint64_t pairs_launches;
    uint64_t pairs_elems;      /* elements summed over those launches */
    double ms_text;            /* first pass, rs_scatter_kernel<true> (1 B in, 12 B out) */
    uint64_t text_launches;
    uint64_t mode;             /* how ties were resolved: 0 doubling over an inverse SA (dense), 1 sparse
                                  (hash + key search, no ISA), 2 text rounds only, 3 text rounds then dense */
    uint64_t text_rounds;      /* rounds that extended ties with symbols packed from the text */
    uint64_t big_elems;        /* members of groups > 512 handled by the chained radix sorts, summed */
    uint64_t key_bits;         /* bits of the initial sort key: key_chars * code_bits minus the low bits of the
                                  last symbol that were left out to save a pass */
    /* profile mode: passes of the initial sort, fs_scatter_kernel<KIN, KOUT> (key plane bytes in / out;
     * KIN 0 = packed from the text, KOUT 0 = last pass; values are 4 B in and out, 4 B only out of the
     * text pass).  Index = (KIN / 4) * 3 + KOUT / 4. */
    double fs_ms[9];
    uint64_t fs_launches[9];
    uint64_t fs_elems[9];
    /* initial sort taken by the hybrid MSD path (two global 10-bit partition passes over 8-byte
     * [key | index] elements, then every joint bucket sorted in LDS): 1 when it ran */
    uint64_t msd;
    uint64_t msd_buckets;      /* non-empty joint (20-bit) buckets; filled whenever the path was tried */
    uint64_t msd_max_bucket;   /* largest of them (the path declines above 4088) */
    uint64_t msd_tiles;        /* local-sort workgroups */
    double msd_ms_g1;          /* profile mode: partition scatter from the text (1 B in, 8 B out per suffix) */
    double msd_ms_g2;          /* ... second partition scatter (8 B in, 8 B out) */
    double msd_ms_local;       /* ... local sort (8 B in, 4 B out, sequential) */
    uint64_t msd_slow_tiles;   /* tiles with crowded bins that took the general local-sort kernel */
    /* run-length path (texts made of long runs of equal bytes): the run heads are sorted as a string of one
     * symbol per run, the other suffixes by one short radix sort.  `rounds` etc. then describe the sort of
     * the reduced string. */
    uint64_t runs;             /* maximal runs of equal bytes in the text (always filled) */
    uint64_t rle;              /* 0: not taken; 1: taken, expansion by a stable radix sort; 2: taken, expansion by the
                                  matrix walk (no sort) */
    uint64_t rle_id_bits;      /* key bits of the expansion sort */
    double rle_ms_table;       /* profile mode: run table and symbols */
    double rle_ms_reduced;     /* ... suffix sort of the reduced string */
    double rle_ms_expand;      /* ... expansion and its radix sort */
    /* initial sort taken by the sample sort over 16-byte [key | index] elements (natural text: texts the radix
     * partition above cannot take because some 20-bit prefix holds far more suffixes than a tile): 1 when it ran */
    uint64_t ss;
    uint64_t ss_buckets;       /* non-empty joint buckets */
    uint64_t ss_max_bucket;    /* largest of them (the path declines above 4088: a sampling accident) */
    uint64_t ss_tiles;         /* local-sort workgroups */
    uint64_t ss_samples;       /* sample members the splitters were taken from */
    double ss_ms_sample;       /* profile mode: drawing and sorting the sample */
    double ss_ms_g1;           /* ... first partition (digits from the text, scatter: 3 B in, 2 + 16 B out per suffix) */
    double ss_ms_g2;           /* ... second partition (digits 16 in / 2 out, scatter 18 in / 16 out) */
    double ss_ms_local;        /* ... local merge sort (16 B in, 4 B out) */
    double ms_initial;         /* device time from the start of the build to the end of the initial sort (always filled) */
    uint64_t period;           /* word length p when the head of the text repeats one word of 2 .. 1024 bytes (else 0) ... */
    uint64_t period_extent;    /* ... how far that repetition reaches from the start of the text ... */
    uint64_t period_path;      /* ... 1: it covers the text (at most 1024 bytes behind it) and the suffix array was written
                                  in closed form (rle_build.h): rotation blocks + a host sort of the last few suffixes */
    uint64_t plan_hint;        /* 0: the sizing sample chose the initial sort; 1: the previous build on this device sorted
                                  the same kind of text (same byte values, same size class) with the MSD sort and this
                                  build went straight to it (PSS_NO_PLAN_CACHE=1: never); 2: ... and recoded the text with
                                  the remembered alphabet inside the sort's first pass, without an alphabet pass of its
                                  own (the pass checks that every byte has a code; PSS_NO_PLAN_FRONT=1: never); 3: no
                                  plan, but the chunk's own symbol counts are close to uniform (sum p^2 < 0.035: log lines,
                                  identifiers -- not natural language) and it went to the MSD sort the same way, without
                                  recode pass and sizing sample */
    /* anchor round (ties that outlive the text rounds -- duplicated stretches of text -- are resolved by ONE round
     * keyed by the ranks of a content-defined sample of positions, the anchors, instead of log2(repeat length) rank
     * rounds over the whole text; anchor_impl.h) */
    uint64_t anchor;           /* 1 when it ran */
    uint64_t anchor_omega;     /* window of the minimizers (every window of this many positions holds an anchor) */
    uint64_t anchor_w;         /* bytes hashed per position */
    uint64_t anchor_count;     /* anchors (also filled when the path declined: more than n / 5) */
    uint64_t anchor_active;    /* suffixes still tied when the round ran */
    uint64_t anchor_depth;     /* symbols every tied group shared at that point */
    uint64_t anchor_text_rounds; /* text rounds of the anchors' own sort (names of 2 omega + w - 1 symbols) */
    uint64_t anchor_rounds;    /* rank rounds over the string of anchor names */
    uint64_t anchor_sum_active;  /* anchors still tied, summed over those rounds */
    uint64_t anchor_left;      /* suffixes the round left tied (always 0; a non-zero value is an internal error that the
                                  rank rounds then repair) */
    uint64_t anchor_levels;    /* anchor levels stacked: 1 = anchors of the text; 2 = anchors of the string of their names, ... */
    uint64_t probe_pairs;      /* before the first text round: neighbours of the active list sampled from one group ... */
    uint64_t probe_same;       /* ... and those that share 48 more symbols (most of them: the ties are repeats, no text round) */
    uint64_t periodic_rounds;  /* rank rounds (of any anchor level) in which large groups took the periodic key: members of a run of
                                  period p <= h ordered by how far the period goes on and how it breaks, not by ISA[i + h] */
    uint64_t periodic_members; /* ... and the members of those groups, summed over the rounds */
    uint64_t ss_planned;       /* 1: the sample sort cut this chunk with the sorted sample of the previous chunk of the same
                                  size and alphabet (no sample of its own, no sizing sample: plan_hint = 1 with ss = 1) */
    uint64_t dup_screen;       /* first chunk with log-like symbol counts: places among 8192 sampled ones whose 16 bytes occur at an
                                  earlier sampled place too (>= 8: copies, no shortcut to the MSD sort) */
    uint64_t ss_plan_refused;  /* 1: the previous chunk's sample left a bucket beyond a tile; the build started over
                                  without the plan (the attempt is part of ms_total, ms_restarts), later chunks wait before they try */
    uint64_t ss_declined_nomem; /* 1: no room in HBM for the sample sort's two 16 n-byte element buffers -- the build went on
                                  with the LSD passes instead of failing */
    uint64_t anchor_side;      /* 1: the anchors were selected and sorted BESIDE the text round that precedes the anchor round (second
                                  stream, second host thread: sa_build.hip, SideAnchors); 2: started so, and thrown away */
    double anchor_ms;          /* device time of the anchors' selection and sort */
    double ms_restarts;        /* part of ms_total: attempts given up (a remembered plan, or the shortcut of a first chunk, that
                                  this text did not fit -- the build started over without it) */
    uint64_t msd_lookback;     /* 1: the MSD sort took its two digits in LSD order and partitioned the second pass in one sweep
                                  (decoupled look-back, no second histogram pass: round 6; texts below 2^30 bytes) */
    uint64_t msd_finished;     /* suffixes of small tie groups that the MSD sort's finishing kernel placed for good with one more
                                  64-bit text key (msd_sort.hip, msd_finish_kernel); rounds / sum_active count what was left */
} pss_sa_stats;

/*
 * Drop-in for `libsais(T, SA, n, 0, NULL)` as called by
 * construct_suffix_array (src/lib.rs:24-40; contract src/libsais/libsais.h:57-65,
 * src/libsais/libsais.c:6597-6610): SA[0..n) becomes the permutation of 0..n-1
 * that orders the suffixes of T by unsigned bytes, a proper prefix first.
 * n == 0 writes nothing, n == 1 writes SA[0] = 0.  T and SA are HOST pointers;
 * the text is uploaded, sorted on `device` and the result copied back.
 * Returns 0, PSS_EINVAL (NULL pointers, n < 0), PSS_ENOMEM or PSS_EDEVICE.
 */
int32_t pss_sa_build(const uint8_t *T, int32_t *SA, int32_t n, int32_t device);

/* Same, with T and SA already resident in the HBM of `device` (T must be
 * readable for n bytes, SA writable for n int32).  `flags` bit 0 = profile
 * mode (per-pass HIP events, fills ms_sort); bit 1 = build without any plan
 * shortcut (internal: restarts); bit 2 = no shortcut from the symbol counts of a
 * first chunk (internal: restarts); bit 3 = forget what earlier builds on this
 * device left behind first (a COLD build: what the first chunk of a corpus sees;
 * bench.py's value_cold).  This is the timed region of bench.py: inputs resident,
 * no PCIe. */
#define PSS_SA_PROFILE 1u                   /* bit 0 */
#define PSS_SA_NO_PLAN 2u                   /* bit 1 */
#define PSS_SA_NO_FIRST_CHUNK_SHORTCUT 4u   /* bit 2 */
#define PSS_SA_COLD 8u                      /* bit 3 */
int32_t pss_sa_build_device(const void *d_T, void *d_SA, int32_t n, int32_t device,
                            uint32_t flags, pss_sa_stats *stats);

/* The builder's device radix sort on its own (test / measurement utility, no
 * reference counterpart): stable LSD sort of n (u64 key, u32 value) pairs by the
 * key bits [0, key_bits), in place, all pointers resident on `device`.
 * *ms_scatter (optional) receives the summed HIP-event time of the scatter kernel. */
int32_t pss_sort_pairs_device(void *d_keys, void *d_vals, uint32_t n, int32_t key_bits, int32_t device,
                              double *ms_scatter);

/* The same sort with its pass mask and its range cap exposed (test / measurement utility, no
 * reference counterpart): the pairs are ordered by the 8-bit digits p < ceil(key_bits / 8) whose bit
 * (1 << p) is set in pass_mask, least significant first -- every other bit of a key is ignored.
 * Stable for n > 4096; up to 4096 pairs equal keys leave in value order.  A pass is cut into at most
 * max_ranges workgroup ranges (a multiple of 8 in 8 .. 1024; the builder always uses 1024): a small cap
 * makes a range hold several 4096-pair tiles at a small n.  The result is in the caller's buffers.
 * PSS_EINVAL before any device is touched: NULL pointers with n > 0, key_bits outside 1 .. 64, a bad cap. */
int32_t pss_sort_pairs_ex_device(void *d_keys, void *d_vals, uint32_t n, int32_t key_bits, uint32_t pass_mask,
                                 uint32_t max_ranges, int32_t device);

/* The builder's initial LSD sort of all n suffixes on its own (test / measurement utility, no reference
 * counterpart).  d_codes: the recoded text on `device`, 16-byte aligned, readable for n + 64 bytes and
 * padded by the caller.  The key of suffix i is its key_chars symbols of code_bits bits each, first symbol
 * highest, zero past the end of the text (plus_one: symbol = byte + 1 inside the text), shifted right by
 * `drop`; the suffixes are sorted by the whole 8-bit digits of it that cover its low key_bits bits, that is
 * by its low 8 * ceil(key_bits / 8) bits (a build's key has no bits above key_bits; a smaller key_bits gives
 * every prefix of a build's passes).  Equal keys are left in the order the pass over the text ranks them --
 * inside a tile of 4096 by (wave, round r of the thread's 16 suffixes, lane), not by index -- which every
 * later pass keeps.  d_out receives n u32.
 * carry_flags = 1: the flag-carrying passes -- suffix indices, bit 31 set when the key (those bits of it)
 * equals the predecessor's.  carry_flags = 0: the plain passes with the text as source, plain indices.
 * max_ranges: as for pss_sort_pairs_ex_device.
 * PSS_EINVAL before any device is touched: NULL or misaligned pointers, n >= 2^31, code_bits outside
 * 1 .. 9, key_chars outside 1 .. 16, key_chars * code_bits > 64, drop outside 0 .. code_bits - 1, key_bits
 * outside 9 .. 64 with flags or 1 .. 64 without, key_bits > key_chars * code_bits - drop, a bad cap. */
int32_t pss_suffix_sort_device(const void *d_codes, uint32_t n, int32_t code_bits, int32_t key_chars, int32_t plus_one,
                               int32_t drop, int32_t key_bits, int32_t carry_flags, uint32_t max_ranges, void *d_out,
                               int32_t device);

/* ---- Writer (src/lib.rs:42-144; pysubstringsearch/__init__.py:6-41) ----- */

/* Writer::new, src/lib.rs:50-65.  Creates/truncates `path`.  max_chunk_len < 0
 * means None (512 MiB, src/lib.rs:57).  Suffix arrays are built on `device`. */
int pss_writer_open(const char *path, int64_t max_chunk_len, int32_t device, pss_writer **out);
/* The same with the container format chosen (no reference counterpart).
 * 1 = the reference's records, u32le len | text | u32le 4n | n x i32le (src/lib.rs:112-119), whose
 *     u32 at lib.rs:116 limits a chunk to < 1 GiB of text;
 * 2 = "PSSIDX\x02\x00" | u32le flags (0) | u32le reserved (0), then records with 64-bit lengths,
 *     u64le n | text | u64le 4n | n x i32le: chunks of up to 2^31 - 1 bytes (max_chunk_len beyond
 *     that is PSS_EINVAL).  pss_reader_open recognises either format by the magic.
 * 2 | PSS_FORMAT_STRIPED (round 5) = format 2 with header flags bit 0 set (bits 8..15: S, bits 16..23: log2 of the
 *     unit, 24): the records hold no suffix arrays (u64le n | text | u64le 4n), the arrays live in S files
 *     `<path>.sa0` .. `<path>.sa<S-1>` (S = 8; PSS_STRIPES) -- every chunk's array starts a new 16 MiB unit, unit u
 *     sits in file u mod S at offset (u / S) * 16 MiB -- and are written and read by several threads, a file each:
 *     one file in the page cache takes 11 - 14 GB/s on the test box whatever the number of writers, a file per
 *     writer 47 - 97.  The stripe files travel with the index file; pss_reader_open reads the flag. */
#define PSS_FORMAT_STRIPED 0x100
int pss_writer_open_format(const char *path, int64_t max_chunk_len, int32_t device, int32_t format_version,
                           pss_writer **out);
/* The same over several devices ("each GPU builds its chunks; host writes records in chunk
 * order"): chunk k of the file is built on devices[k % n_devices], up to 2 n_devices chunks are in flight
 * (G being built, the records of the earlier ones streaming to the file in chunk order), and the file
 * is byte-identical to the single-device one.  The reference builds one chunk at a time inside
 * dump_data (src/lib.rs:105-124).  The same device may be listed more than once. */
int pss_writer_open_multi(const char *path, int64_t max_chunk_len, const int32_t *devices, int32_t n_devices,
                          int32_t format_version, pss_writer **out);
/* Writer::add_entry, src/lib.rs:88-103.  PSS_ETOOBIG when len > limit. */
int pss_writer_add_entry(pss_writer *w, const uint8_t *text, uint64_t len);
/* Writer::add_entries_from_file_lines, src/lib.rs:67-86 (bstr for_byte_line rule). */
int pss_writer_add_file_lines(pss_writer *w, const char *path);
/* Writer::dump_data, src/lib.rs:105-124: emits u32le len | data | u32le 4n | n x i32le. */
int pss_writer_dump(pss_writer *w);
/* Writer::finalize, src/lib.rs:126-135. */
int pss_writer_finalize(pss_writer *w);
/* Drop for Writer, src/lib.rs:138-144: finalize, close the file, free. */
int pss_writer_close(pss_writer *w);
/* Current chunk limit (Vec capacity in the reference, src/lib.rs:62,75,92,96). */
uint64_t pss_writer_chunk_limit(const pss_writer *w);
/* Which way the bytes went (round 5; diagnostics, nothing a caller must look at): records written through a shared
 * mapping of the index file (tmpfs; PSS_WRITER_MMAP=0|1 overrides, PSS_WRITER_MMAP_MIN = smallest such record, default
 * 1 MiB) or pwritten; bytes of pss_writer_add_file_lines input read straight into the chunk or through a block buffer
 * (lines with a '\r', lines that do not fit the chunk any more). */
typedef struct pss_writer_io {
    uint64_t records_mapped;
    uint64_t records_pwritten;
    uint64_t ingest_direct_bytes;
    uint64_t ingest_copied_bytes;
} pss_writer_io;
int pss_writer_io_stats(pss_writer *w, pss_writer_io *out);

/* ---- Reader (src/lib.rs:146-288; pysubstringsearch/__init__.py:44-73) --- */

/* Reader::new, src/lib.rs:162-199.  Parses the chunk records of `path` (the reference
 * container, or format 2 -- recognised by its magic, see pss_writer_open_format) and
 * makes the text AND suffix array of every chunk c with
 * c % shard_count == shard_index resident on `device`: in HBM, the suffix arrays
 * beyond the HBM budget in pinned host memory (pss_reader_residency)
 * (shard_index 0, shard_count 1 = whole file).  Every resident chunk also gets a
 * table of key samples (first 8 bytes of every 2048th suffix) that the searches
 * consult before the suffix array. */
int pss_reader_open(const char *path, int32_t device, int32_t shard_index, int32_t shard_count,
                    pss_reader **out);
/* The same over several devices in ONE process, no launcher, no torch (the reference fans a search over all chunks
 * inside the process too: rayon, src/lib.rs:207, 280-284): chunk c of the file becomes resident on
 * devices[c % n_devices]; every device answers a batch for its chunks on a thread of its own and the results are
 * merged on the host (query-major, device-major inside a query).  The same ordinal may be listed more than once
 * ("virtual devices": the parts then take turns on that GPU).  pss_reader_search_batch / count_batch / residency /
 * evict / promote work on such a reader; the device-resident result and the chunk hand-off calls do not. */
int pss_reader_open_multi(const char *path, const int32_t *devices, int32_t n_devices, pss_reader **out);
/* Observer of the placement above: the number of parts of the reader (1 for a single-device reader) and, in counts[0 .. cap),
 * how many chunks each part holds -- chunk c of the file lives in part c % G, so 15 chunks over 8 devices read
 * 2,2,2,2,2,2,2,1 ("report this imbalance").  No reference counterpart. */
uint64_t pss_reader_part_chunks(const pss_reader *r, uint64_t *counts, uint64_t cap);

/* Residency manager ("LRU when index > HBM"; the reference keeps every suffix array on disk,
 * src/lib.rs:179-189).  A reader whose suffix arrays do not all fit the HBM budget keeps a decayed per-chunk count of the
 * hits its batches find and, between batches, lets the hottest suffix array of the host tier change places with the
 * coldest one in HBM when it is more than twice as hot (at most one exchange per batch).  On by default
 * (PSS_READER_AUTO_RESIDENCY=0 or on = 0: off); pss_reader_evict_chunk / promote_chunk remain as explicit overrides.
 * pss_reader_chunk_tiers: tiers[c] = 0 (suffix array of chunk c in HBM) or 1 (pinned host memory), for the first `cap`
 * chunks; *auto_moves = exchanges / promotions the manager has made so far. */
int pss_reader_set_auto_residency(pss_reader *r, int32_t on);
int pss_reader_chunk_tiers(const pss_reader *r, uint8_t *tiers, uint64_t cap, uint64_t *auto_moves);
/* Residency control: move the suffix array of resident chunk `index` (file order) out of HBM into
 * pinned host memory, where the kernels read it over PCIe (evict), or back (promote; PSS_ENOMEM when HBM has no
 * room).  Text and key samples stay in HBM.  No-ops when the chunk already is where it is asked to be. */
int pss_reader_evict_chunk(pss_reader *r, uint64_t index);
int pss_reader_promote_chunk(pss_reader *r, uint64_t index);
/* Low-latency mode for single queries (off by default; single-device readers).  Launching a kernel and waiting for its
 * completion are about half of what one query costs (~10 of ~22 us); with this mode on, the first single query of a
 * burst starts a RESIDENT search kernel -- one workgroup per chunk that waits for queries in a mailbox in
 * pinned host memory -- and the following ones are posted there and answered without a launch (results are the same
 * bytes either way).  The kernel holds a lease, not the GPU: it leaves by itself after PSS_RESIDENT_IDLE_US (1000)
 * without a query and after PSS_RESIDENT_LIFE_US (50000) in any case, so a crashed host or a device-wide
 * synchronisation elsewhere in the process waits no longer than that; the next single query starts another.  Batches,
 * counts, device-resident results, queries with more hits than the path holds, and every call that changes the
 * reader's chunks go through the ordinary path (and stop the kernel where they must).  While it waits, the kernel
 * occupies one workgroup slot per chunk (a chunk with more than 1024 hits sends the query to the ordinary path) and nothing
 * else.  pss_reader_low_latency_stats: kernels started / queries answered by one, per device. */
int pss_reader_set_low_latency(pss_reader *r, int32_t on);
int pss_reader_low_latency_stats(const pss_reader *r, uint64_t *launches, uint64_t *served);
/* Order of the entries INSIDE one chunk's share of a query (round 5).  The reference walks the hits of a chunk in
 * suffix-array order and pushes an entry when its line start is first seen (src/lib.rs:262-276): a chunk's entries come
 * out in suffix-array order of their FIRST hit.  The default here (PSS_ORDER_TEXT) keeps the leftmost match of every
 * entry and lists the entries in suffix-array order of THAT match -- the same multiset (what the reference's tests
 * compare, tests/test_pysubstringsearch.py:32-37), possibly another order when an entry holds the pattern twice.
 * PSS_ORDER_SA reproduces the reference's list element by element (chunks in index order; the reference's order between
 * chunks is whatever its thread pool makes of it, src/lib.rs:207,280).  It takes the general pipeline and one more
 * sort of the hits: batches pay a few per cent, a single query loses the fused path.  PSS_RESULT_ORDER=sa in the
 * environment makes it the default of every reader opened afterwards. */
#define PSS_ORDER_TEXT 0
#define PSS_ORDER_SA 1
int pss_reader_set_result_order(pss_reader *r, int32_t order);
int32_t pss_reader_result_order(const pss_reader *r);
/* An empty reader on `device`, to be filled with pss_reader_add_chunk_device
 * (Writer -> Reader hand-off through HBM, no file). */
int pss_reader_create(int32_t device, pss_reader **out);
/* Adopts COPIES of a device-resident chunk (text n bytes, SA n int32). */
int pss_reader_add_chunk_device(pss_reader *r, const void *d_text, const void *d_sa, uint32_t n);
/* Replaces resident chunk `index` (index == num_chunks appends) by a copy of
 * the device-resident chunk; reuses the HBM allocation when the size matches
 * (re-indexing the same shard repeatedly without allocator traffic). */
int pss_reader_set_chunk_device(pss_reader *r, uint64_t index, const void *d_text, const void *d_sa, uint32_t n);
/* Chunks resident in this reader. */
uint64_t pss_reader_num_chunks(const pss_reader *r);
/* Where the resident index lives.  The text of every chunk is in HBM; a suffix array is too while it
 * fits (PSS_READER_HBM_BUDGET bytes when set, else until 2 GiB of HBM are left), otherwise it stays in
 * pinned host memory and the kernels read it over PCIe (the key samples in HBM confine a query to a few
 * dozen such reads).  host_chunks = chunks whose suffix array is on the host.  No reference counterpart:
 * Reader::new keeps the text in RAM and every suffix array on disk (src/lib.rs:176-189). */
int pss_reader_residency(const pss_reader *r, uint64_t *hbm_bytes, uint64_t *host_bytes, uint64_t *host_chunks);

/* Per-batch statistics of the last pss_reader_search_batch call. */
typedef struct pss_search_stats {
    uint64_t queries;
    uint64_t hits;          /* suffix-array hits before per-chunk dedupe */
    uint64_t entries;       /* entries returned */
    uint64_t result_bytes;
    double ms_device;       /* HIP-event time of the kernels of the batch */
    double ms_interval;     /* ... of the interval-search kernel alone */
    double ms_host;         /* wall time of the whole batch inside the library (host clock) */
    uint32_t route;         /* PSS_ROUTE_* bits: which search routes served the batch (a multi-device reader: OR of its devices) */
    uint32_t route_pad;
} pss_search_stats;

/* Bits of pss_search_stats.route.  A batch that one route could not finish names every route it went through: e.g.
 * SMALL_BLOCK | SMALL_OVERFLOW | INTERVAL_WAVE | MID for a fused launch over its capacities that the mid pipeline took. */
#define PSS_ROUTE_RESIDENT        0x0001u  /* the resident low-latency kernel answered (pss_reader_set_low_latency) */
#define PSS_ROUTE_SMALL_BLOCK     0x0002u  /* fused path, one to 32 workgroups per (query, chunk) pair */
#define PSS_ROUTE_SMALL_WAVE      0x0004u  /* fused path, one wavefront per pair */
#define PSS_ROUTE_SMALL_OVERFLOW  0x0008u  /* the fused path ran over a capacity; a later route took the batch */
#define PSS_ROUTE_INTERVAL_LANE   0x0010u  /* interval search, one lane per pair */
#define PSS_ROUTE_INTERVAL_GROUP  0x0020u  /* interval search, 16 lanes per pair */
#define PSS_ROUTE_INTERVAL_WAVE   0x0040u  /* interval search, one wavefront per pair */
#define PSS_ROUTE_KEY_SAMPLES     0x0080u  /* the reader's chunks have key-sample tables (the searches start from a window) */
#define PSS_ROUTE_MID             0x0100u  /* mid pipeline */
#define PSS_ROUTE_MID_OVERFLOW    0x0200u  /* the mid pipeline ran over its hits or bytes; the general pipeline took the batch */
#define PSS_ROUTE_GENERAL         0x0400u  /* general multi-kernel pipeline */
#define PSS_ROUTE_SA_ORDER        0x0800u  /* ... with the suffix-array result order (pss_reader_set_result_order) */
#define PSS_ROUTE_COUNTS          0x1000u  /* ... counting entries only (pss_reader_count_batch) */
#define PSS_ROUTE_ANCHORED        0x2000u  /* ... of an anchored batch (pss_reader_search_anchored_batch) */

/*
 * Reader::search (src/lib.rs:201-287) for a whole batch in one call, i.e.
 * Reader.search_multiple (pysubstringsearch/__init__.py:61-73): query q is
 * qbytes[qoffsets[q] .. qoffsets[q+1]).  For every query and every resident
 * chunk: the maximal suffix-array interval whose suffixes start with the
 * query (src/lib.rs:209-252), the entry around each hit (newline scan,
 * src/lib.rs:266-273), deduplicated per (query, chunk) on the entry's start
 * offset (src/lib.rs:262,274).  Entries come back query-major (all entries of
 * query 0, then query 1, ...), inside a query chunk-major.
 */
int pss_reader_search_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets,
                            uint32_t nq, pss_result **out);
/*
 * Beyond the reference surface: counts[q] = the number of
 * entries pss_reader_search_batch would return for query q (after the per-chunk
 * dedupe), without materialising a single entry -- the interval search, the
 * dedupe flags and two scans; nothing but nq counters crosses PCIe.  For
 * high-hit queries this is the part of Reader::search (src/lib.rs:254-278) that
 * dominates on the CPU (README.md:57).
 */
int pss_reader_count_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets,
                           uint32_t nq, uint64_t *counts);
/*
 * Entry ids (no reference counterpart: Reader::search hands out entry text only, src/lib.rs:254-286).  An entry id is
 * (chunk index in the index file << 32) | line, line = the number of 0x0A bytes in the chunk's text before the entry's
 * first byte; a chunk holds count(0x0A) + (1 when it is non-empty and does not end in 0x0A) entries, empty ones
 * included.  A sharded or multi-device reader hands out the chunk's index IN THE FILE, so the ids of one file mean the
 * same everywhere; a reader filled by pss_reader_add_chunk_device numbers its chunks as they were added.  For a
 * whole-file reader, (entries of the chunks before c) + line is the entry's 0-based position in the order the entries
 * were added -- the line number in the source file for an index made by one pss_writer_add_file_lines call.
 * The ids rest on a line index per chunk (one u32 newline rank per 256 bytes of text, 1/64 of the text, in HBM) that is
 * built by the first of these three calls on a reader -- and again for a chunk that is replaced or appended; a
 * reader that never asks for ids allocates nothing for it.  From then on pss_reader_residency counts it in hbm_bytes.
 *
 * pss_reader_search_ids_batch: the ids of the entries pss_reader_search_batch would return, in the same order (the
 * reader's result order included).  *out is a pss_result whose query_counts are the entries per query and whose bytes
 * are num_entries little-endian u64 ids, 8-byte aligned (offsets[i] = 8 * i).  The batch takes the general pipeline as
 * pss_reader_count_batch does -- interval search, dedupe, one scan -- and then writes one id per entry: no entry text is
 * measured, copied or brought down.
 */
int pss_reader_search_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                pss_result **out);
/* Text of the entries ids[0 .. n): a packed result of n "queries" with one entry each, in the order asked.
 * PSS_EINVAL (message in pss_last_error, *out untouched) when an id names a chunk this reader does not hold or a
 * line the chunk does not have.  The same id may be asked for more than once. */
int pss_reader_entries_by_id(pss_reader *r, const uint64_t *ids, uint64_t n, pss_result **out);
/*
 * Anchored search (no reference counterpart: Reader::search answers "contains" only).  Which entries START WITH the
 * pattern, END WITH it, or EQUAL it -- exact bytes, as everywhere.  anchors[q] is PSS_ANCHOR_START, PSS_ANCHOR_END or
 * both, one value per query, so one batch may mix the three kinds.  With s the start of an entry and e the position of
 * its closing 0x0A (or the length n of the chunk's text when none follows; the entries are those of "Entry ids" above),
 * a pattern of m bytes matches the entry when
 *   PSS_ANCHOR_START                   text[s, s + m) == pattern and s + m <= e,
 *   PSS_ANCHOR_END                     text[e - m, e) == pattern and e - m >= s,
 *   PSS_ANCHOR_START | PSS_ANCHOR_END  e - s == m and text[s, e) == pattern.
 * Every entry matches at most once.  The empty pattern matches every entry under START and under END, and the empty
 * entries under both.  A pattern that holds 0x0A matches nothing.  The text handed out for a matching entry is what
 * pss_reader_search_batch hands out for a hit in it (an unterminated last entry loses its last byte); the ids are
 * those of pss_reader_search_ids_batch.
 * The search is the interval search of pss_reader_search_batch on "\n" + pattern, pattern + "\n" or
 * "\n" + pattern + "\n" -- an interval of exactly one hit per matching entry -- plus at most two hits per chunk that no
 * newline delimits: its first entry and an unterminated last one.  The work follows the answer, not the number of
 * occurrences of the pattern, and nothing is deduplicated.
 * Order: query-major, chunk-major inside a query; inside one (query, chunk) pair deterministic and the same for the
 * text and the id variant, otherwise unspecified -- pss_reader_set_result_order has no effect (one hit per entry).
 * An anchors[q] of 0 or above 3 is PSS_EINVAL (message in pss_last_error, *out untouched); anchor 0 is what
 * pss_reader_search_batch is for.  Whole-file, sharded and multi-device readers, and suffix arrays on the host tier,
 * are served alike.  pss_reader_last_stats: hits = interval hits + chunk-edge hits; route = GENERAL | ANCHORED | the
 * interval bits (| COUNTS for the count call).  The id variant builds the line tables on first use, the other two
 * allocate nothing for them.
 * Out of scope: the fused small-batch path and the resident low-latency kernel (an anchored batch always takes the
 * general pipeline, as an id batch does), a device-resident result (pss_reader_search_batch_device), and the multi-process
 * gather over RCCL (dist.ShardedReader).
 */
#define PSS_ANCHOR_START 1u
#define PSS_ANCHOR_END   2u
/* packed entry text, as pss_reader_search_batch */
int pss_reader_search_anchored_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                     const uint8_t *anchors, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_anchored_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                         const uint8_t *anchors, pss_result **out);
/* counts[q] = entries query q matches; nothing but nq counters comes down */
int pss_reader_count_anchored_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                    const uint8_t *anchors, uint64_t *counts);
/*
 * All-terms search (no reference counterpart): which entries contain ALL of some terms and NONE of some others, e.g.
 * "error" and "timeout" but not "retry".  The batch holds ngroups GROUPS.  Group g is the terms group_offsets[g] ..
 * group_offsets[g + 1] of the nterms terms packed in tbytes / toffsets (as queries are everywhere); exclude[t] = 0 makes
 * term t an INCLUDE term, 1 an EXCLUDE term.  An entry of a chunk matches a group when every include term occurs in it
 * and no exclude term does, where "occurs in" is what pss_reader_search_batch means: the entry is among the entries that
 * call returns for the term alone (exact bytes, the whole entry, the last byte of an unterminated last entry included).
 * The answer for a group is therefore the intersection of its include terms' pss_reader_search_ids_batch results minus
 * the union of its exclude terms'.  A term may be repeated; a term both included and excluded gives an empty answer.  An
 * include term that holds 0x0A makes its group match nothing; an exclude term that holds 0x0A excludes nothing.
 * *out has one row ("query") per GROUP: query_counts[g] entries, packed as pss_reader_search_batch (text; an unterminated
 * last entry loses its last byte) or pss_reader_search_ids_batch (ids) pack them; counts[g] likewise.
 * PSS_EINVAL (message in pss_last_error, *out untouched): a group without an include term ("everything except" is not a
 * search), an empty term, an exclude[t] other than 0 or 1, group offsets that do not start at 0, decrease or do not end
 * at nterms, a null group_offsets / out, a null tbytes / toffsets / exclude with nterms > 0, a null reader.  The batch
 * is checked before the reader: a malformed batch is reported as such even when r is null, a null r after that.
 * The search: the interval search of pss_reader_search_batch over all (term, chunk) pairs gives every term's
 * occurrences per chunk; per (group, chunk) pair the include term with the fewest (the lowest index on a tie) DRIVES
 * the general pipeline as a plain query would, and each candidate entry it yields is scanned once for the group's other
 * terms.  The work follows the rarest include term, and a chunk in which any include term is absent contributes nothing
 * without a hit being looked at.
 * Order: group-major, chunk-major inside a group; inside one (group, chunk) pair the plain search's default order for
 * the driver term, the same for the text and the id variant -- pss_reader_set_result_order has no effect.  A group of one
 * include term and no exclude term returns exactly what pss_reader_search_ids_batch returns for that term under the
 * default order.
 * Whole-file, sharded and multi-device readers, and suffix arrays on the host tier, are served alike.
 * pss_reader_last_stats: queries = groups, hits = the sum of the drivers' interval hits, entries = what is returned;
 * route = GENERAL | the interval bits (| COUNTS for the count call) -- there is no bit of its own.  The id variant builds
 * the line tables on first use, the other two allocate nothing for them.
 * Out of scope: the fused small-batch path and the resident low-latency kernel, the mid pipeline (an all-terms batch
 * always takes the general pipeline), a device-resident result (pss_reader_search_batch_device), and the multi-process
 * gather over RCCL (dist.ShardedReader).
 */
/* packed entry text, one row per group */
int pss_reader_search_terms_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms,
                                  const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *exclude, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_terms_ids_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms,
                                      const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *exclude, pss_result **out);
/* counts[g] = entries group g matches; nothing but ngroups counters comes down */
int pss_reader_count_terms_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms,
                                 const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *exclude, uint64_t *counts);
/*
 * Wildcard search (no reference counterpart): which entries hold these pieces IN THIS ORDER -- SQL's LIKE 'GET %/admin% 500',
 * a shell glob whose only wildcard is `*`.  The batch holds ngroups SEQUENCE GROUPS.  Group g is the ordered list of the
 * k >= 1 non-empty SEGMENTS group_offsets[g] .. group_offsets[g + 1] of the nsegs segments packed in sbytes / soffsets (as
 * queries are everywhere), s_0 .. s_{k-1}, and the anchor byte anchors[g]: 0, PSS_ANCHOR_START, PSS_ANCHOR_END or both.
 * An entry is the bytes [start, end) of a chunk's text, end = its closing 0x0A or the length n of the text when none
 * follows; the last byte of an unterminated last entry TAKES PART in the match, exactly as in the all-terms search,
 * although the text handed out loses it.  The entry matches the group when positions p_0 < p_1 < .. < p_{k-1} exist with
 *   entry[p_j, p_j + |s_j|) == s_j                for every j,
 *   p_{j+1} >= p_j + |s_j|                        in order, no overlap,
 *   p_0 == start                                  when PSS_ANCHOR_START is set,
 *   p_{k-1} + |s_{k-1}| == end                    when PSS_ANCHOR_END is set.
 * As a glob:  0: *s0*s1*..*   START: s0*s1*..*   END: *s0*..*sk-1   START | END: s0*..*sk-1.  With k = 1 and both anchors
 * the entry equals s_0; with k = 1 and no anchor this is pss_reader_search_batch's "contains".  `a*a` does not match the
 * entry `a`.  A segment that holds 0x0A makes its group match nothing.  Every entry appears at most once per group.
 * *out has one row ("query") per GROUP, packed as the all-terms calls pack theirs (text or ids); counts[g] likewise.
 * PSS_EINVAL (message in pss_last_error, *out / counts untouched): a group without a segment, an empty segment, an
 * anchor byte with bits other than START | END, group offsets that do not start at 0, decrease or do not end at nsegs, a
 * null group_offsets / anchors / out, a null sbytes / soffsets with nsegs > 0, a null reader (judged last, as for the
 * all-terms calls).
 * The search: the all-terms search up to its verify step -- the interval search over all (segment, chunk) pairs, per
 * (group, chunk) pair the segment with the fewest occurrences (the lowest index on a tie) DRIVES, one candidate per entry
 * that holds it -- then every candidate entry is walked once, left to right: the anchored segments are pinned to the
 * entry's ends and each remaining segment takes its leftmost occurrence behind the one before it.  Leftmost-greedy is
 * complete when `*` is the only wildcard.  A chunk that lacks any segment contributes nothing without a hit being looked at.
 * Order: group-major, chunk-major inside a group; inside one (group, chunk) pair the plain search's default order for the
 * driver segment, the same for the text and the id variant -- pss_reader_set_result_order has no effect.  A group of one
 * segment and no anchor returns exactly what pss_reader_search_ids_batch returns for it under the default order.
 * Whole-file, sharded and multi-device readers, and suffix arrays on the host tier, are served alike.
 * pss_reader_last_stats: queries = groups, hits = the sum of the drivers' interval hits, entries = what is returned;
 * route = GENERAL | the interval bits (| COUNTS for the count call) -- there is no bit of its own.  The id variant builds
 * the line tables on first use, the other two allocate nothing for them.
 * Out of scope: exclusions inside a group (`?` and byte classes are pss_reader_search_seqc_batch's, below); driving an anchored first or last segment through
 * the anchored search's "\n" + s rewrite (`a*` follows the occurrences of `a`, not the entries that start with it); the
 * fused, resident and mid paths; a device-resident result; the multi-process gather over RCCL (dist.ShardedReader).
 */
/* packed entry text, one row per group */
int pss_reader_search_seq_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs,
                                const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_seq_ids_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs,
                                    const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, pss_result **out);
/* counts[g] = entries group g matches; nothing but ngroups counters comes down */
int pss_reader_count_seq_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs,
                               const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, uint64_t *counts);
/*
 * Wildcard search with byte classes (no reference counterpart): pss_reader_search_seq_batch whose segments hold, beside
 * literal bytes, positions that accept ONE BYTE OUT OF A SET -- a glob's `?` and `[0-9]`, `[!x]`.  One family of three calls
 * serves exact bytes and, with PSS_SEQ_FOLD in `flags`, the ASCII fold of pss_reader_search_icase_batch.
 * The nsegs segments are packed in sbytes / soffsets as ever, ONE BYTE PER POSITION, and `classes` holds one more byte per
 * position under the same offsets: 0 -- the position is a literal, and sbytes holds its byte --, or k in 1 .. nsets -- the
 * position accepts the bytes of set k, and sbytes holds 0 there.  `sets` is nsets x 32 bytes, nsets <= 255: byte b is in set
 * k iff bit (b & 7) of sets[(k - 1) * 32 + (b >> 3)] is set.  No set holds 0x0A (no entry holds one, so a negated set simply
 * leaves it out), none is empty, and under PSS_SEQ_FOLD every set is closed under the fold: it holds both cases of a letter
 * or neither.  `?` is the set of the 255 bytes other than 0x0A.  Groups and anchors exactly as for the sequence calls.
 * The entry [start, end) matches group g when positions p_0 < p_1 < .. exist as pss_reader_search_seq_batch states them,
 * with "entry[p_j, p_j + |s_j|) == s_j" read position by position: a literal equals the entry's byte (under PSS_SEQ_FOLD:
 * after fold of both), a class position holds it in its set.  |s_j| is the segment's position count: a class position is
 * exactly one byte -- of a UTF-8 character one of several.  A window never reaches the closing 0x0A or past n: a set that
 * holds 0x00 does not match the padding behind a chunk.  A literal 0x0A anywhere in a group makes it match nothing.
 * The CORE of a segment is its longest run of literal positions, the leftmost on a tie (pss_seqc_cores shows it); a segment
 * of class positions alone has none.  The search is the sequence search over the CORES of the segments that have one: the
 * interval search over all (core, chunk) pairs -- under PSS_SEQ_FOLD over the spellings of each core's seed, as
 * pss_reader_search_seq_icase_batch expands a segment --, per (group, chunk) pair the core with the fewest hits (the lowest
 * index on a tie) DRIVES, one candidate per entry that holds it, and every candidate entry is walked once, left to right:
 * each segment at its leftmost place behind the one before it, found by its core and tested at the other positions, the
 * next occurrence of the core on a miss; a segment without a core is tested place by place.  Leftmost-greedy stays
 * complete: every segment has a fixed length.  A chunk that lacks a core contributes nothing without a hit being looked at.
 * Order: group-major, chunk-major; inside a (group, chunk) pair the order the sequence call (under PSS_SEQ_FOLD: its _icase
 * form) has for the driving core as driver segment -- pss_reader_set_result_order has no effect.  A batch without a class
 * position returns exactly what the sequence call returns for it.
 * pss_reader_last_stats: queries = groups, hits = the sum of the driving cores' interval hits (under PSS_SEQ_FOLD: of their
 * seeds' hits), route = GENERAL | the interval bits (| COUNTS) -- no bit of its own.
 * PSS_EINVAL (message in pss_last_error, *out / counts untouched): everything the sequence calls refuse (a null `classes`
 * with nsegs > 0 and a null `sets` with nsets > 0 included); flags other than PSS_SEQ_FOLD; nsets > 255; a class index past
 * nsets; a nonzero byte in sbytes under a class index; a set that holds 0x0A; an empty set; under PSS_SEQ_FOLD a set not
 * closed under the fold; a group none of whose segments has a core (nothing in the suffix array can be looked up for it).
 * The reader is judged last.
 * Out of scope: driving a segment by anything but its longest literal run (a rare byte pair inside it, a set of few bytes);
 * groups without a literal byte; classes in all-terms groups, in the search within k mismatches or edits; POSIX classes
 * such as [:alpha:] (the caller expands them into sets); multi-byte characters; the fused, resident and mid paths; a
 * device-resident result; the multi-process gather over RCCL (dist.ShardedReader).
 */
#define PSS_SEQ_FOLD 1u
/* packed entry text, one row per group */
int pss_reader_search_seqc_batch(pss_reader *r, const uint8_t *sbytes, const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs,
                                 const uint8_t *sets, uint32_t nsets, const uint64_t *group_offsets, uint32_t ngroups,
                                 const uint8_t *anchors, uint32_t flags, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_seqc_ids_batch(pss_reader *r, const uint8_t *sbytes, const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs,
                                     const uint8_t *sets, uint32_t nsets, const uint64_t *group_offsets, uint32_t ngroups,
                                     const uint8_t *anchors, uint32_t flags, pss_result **out);
/* counts[g] = entries group g matches; nothing but ngroups counters comes down */
int pss_reader_count_seqc_batch(pss_reader *r, const uint8_t *sbytes, const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs,
                                const uint8_t *sets, uint32_t nsets, const uint64_t *group_offsets, uint32_t ngroups,
                                const uint8_t *anchors, uint32_t flags, uint64_t *counts);
/* core_off[t] / core_len[t] = the core of segment t of a class plane (core_len 0: none), by the rule the calls above apply.
 * Host only: no device is touched. */
int pss_seqc_cores(const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs, uint32_t *core_off, uint32_t *core_len);
/*
 * Regular-expression search (no reference counterpart): per pattern the entries e -- the bytes [start, end) of a chunk's
 * text as the all-terms search takes them, the last byte of an unterminated last entry included -- for which Python's
 * re.search(pattern, e, re.I if PSS_REGEX_ICASE else 0) finds a match.  A pattern is bytes; the syntax is this subset of
 * `re` over bytes:
 *   literal bytes; `.` (any byte but 0x0A); escaped punctuation; \t \r \n \f \v \a \0 \xHH; \d \D \w \W \s \S (ASCII);
 *   [...] and [^...] with ranges, escapes and \d \w \s inside (a raw byte >= 0x80 inside a set is refused: a set is one
 *   byte, write \xHH); groups ( ) and (?: ), the same thing here; | ; * + ? {m} {m,} {m,n} {,n};
 *   ^ only as the pattern's first byte and $ only as its last: they anchor at the entry's first and last byte; with either
 *   the top level must not be a bare alternation (^a|b is refused, ^(a|b) is the way).
 * Under PSS_REGEX_ICASE only A-Z / a-z fold; a set accepts both cases of the letters written in it and [^a] rejects A.
 * Refused, each with its position in the message: lazy and possessive quantifiers, back-references, look-around,
 * \b \B \A \Z, inline flags and other (?...) forms, named groups, ^ / $ elsewhere, octal escapes, a malformed {} (a literal
 * brace is \{) or [], unbalanced parentheses, groups nested more than 200 deep, an empty pattern, a pattern without a required
 * literal (below).
 * Compilation (host only, csrc/regex_compile.h): Glushkov positions with counted repeats unrolled (more than 2048
 * positions: refused), the 256 bytes partitioned into `classes` classes, and the subset construction of the WHOLE-ENTRY
 * language [^\n]* R [^\n]* -- the leading part dropped under ^, the trailing one under $ -- without minimization.  More than
 * PSS_REGEX_MAX_STATES states: refused ("pattern too complex").  State 0 is dead, the accepting states are >= first_accept,
 * and without $ the one accepting state is `sink`, which absorbs every byte (sink = 0 with $: none).  The table is
 * u16 T[states][classes]; reading byte b in state s leads to T[s * classes + cls[b]].
 * The REQUIRED LITERALS of a pattern are byte runs every match holds: maximal runs of positions written as one byte; of a
 * concatenation its children's and the runs across adjacent literal children, of a group or a repeat with minimum >= 1 the
 * child's, of an alternation or a repeat with minimum 0 none.  Distinct, the longest first (the leftmost on a tie), one
 * that lies inside a longer one dropped, at most 8; folded to lower case under PSS_REGEX_ICASE.  A set or class position is
 * never part of one.
 * The search: the required literals of pattern g are the include terms of all-terms group g (pss_reader_search_terms_batch;
 * under PSS_REGEX_ICASE pss_reader_search_terms_icase_batch) -- the rarest of them per (pattern, chunk) pair drives, one
 * candidate per entry that holds it, entries that lack another literal are dropped --, and every candidate left is walked
 * once through the pattern's table from the entry's first byte to its last (one lane per candidate), stopping at state 0
 * and at sink.  A literal that holds 0x0A makes its pattern match nothing: a count of 0, not an error.  Order and
 * pss_reader_last_stats exactly as the all-terms call has them for those groups (hits = the sum of the drivers' hits; no
 * route bit of its own); pss_reader_set_result_order has no effect.
 * PSS_EINVAL (message in pss_last_error, *out / counts untouched), in this order: a null out / counts, a null pbytes /
 * poffsets with np > 0, flags other than PSS_REGEX_ICASE, offsets that do not start at 0 or that decrease; then the first
 * pattern that does not compile ("pattern <g>: ..."), tables of more than 64 MiB in one batch; a null reader last.  Nothing
 * is launched before all of that has passed.
 * Not built: a table staged in LDS, several lanes per entry, minimization, a cache of compiled patterns (every call
 * compiles its batch), the fused, resident and mid paths, a device-resident result, dist.ShardedReader.
 */
#define PSS_REGEX_ICASE 1u
#define PSS_REGEX_MAX_STATES 4096u
typedef struct pss_regex pss_regex;
typedef struct pss_regex_dfa {
    uint32_t states, classes;
    uint64_t table_bytes;
    uint32_t anchors;                /* PSS_ANCHOR_START | PSS_ANCHOR_END */
    uint32_t start, first_accept, sink;
} pss_regex_dfa;
/* Host only, no device is touched.  *out is freed with pss_regex_free. */
int pss_regex_compile(const uint8_t *pattern, uint64_t len, uint32_t flags, pss_regex **out);
void pss_regex_free(pss_regex *rx);
int pss_regex_info(const pss_regex *rx, pss_regex_dfa *info);
/* The required literals back to back into out[0, cap) and their *count + 1 offsets into offsets[0, 9); PSS_EINVAL when cap
 * is too small.  A literal may be longer than its pattern (`a{200}` has one of 200 bytes: an exact {n} of up to 256 bytes is
 * written out), so ask first: with out = NULL and cap = 0 the call fills offsets and *count alone, and offsets[*count] is the
 * size the buffer needs. */
int pss_regex_literals(const pss_regex *rx, uint8_t *out, uint64_t cap, uint64_t *offsets, uint32_t *count);
/* The device's walk on the host: 1 = bytes[0, len), taken as one entry (it holds no 0x0A), matches, 0 = it does not,
 * PSS_EINVAL for a null argument. */
int pss_regex_match(const pss_regex *rx, const uint8_t *bytes, uint64_t len);
/* packed entry text, one row per pattern */
int pss_reader_search_regex_batch(pss_reader *r, const uint8_t *pbytes, const uint64_t *poffsets, uint32_t np, uint32_t flags,
                                  pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_regex_ids_batch(pss_reader *r, const uint8_t *pbytes, const uint64_t *poffsets, uint32_t np, uint32_t flags,
                                      pss_result **out);
/* counts[g] = entries pattern g matches; nothing but np counters comes down */
int pss_reader_count_regex_batch(pss_reader *r, const uint8_t *pbytes, const uint64_t *poffsets, uint32_t np, uint32_t flags,
                                 uint64_t *counts);
/*
 * Case-insensitive search (no reference counterpart): `grep -i` over the entries.  ASCII only: the bytes 0x41 .. 0x5A (A .. Z)
 * are equivalent to 0x61 .. 0x7A (a .. z), and every other byte -- 0x80 .. 0xFF included, so no letter outside ASCII -- equals
 * only itself; fold(b) maps A .. Z to a .. z.  An entry is the bytes [start, end) of a chunk's text, end = its closing 0x0A or
 * the length n of the text when none follows; the last byte of an unterminated last entry TAKES PART in the match, exactly as
 * in the all-terms and the wildcard search, although the text handed out loses it.  The entry matches pattern p when some m
 * in start .. end - |p| has fold(text[m + i]) == fold(p[i]) for all i.  One row ("query") per pattern, packed as
 * pss_reader_search_batch (text) and pss_reader_search_ids_batch (ids) pack theirs; every entry appears at most once per
 * pattern.  A pattern that holds 0x0A matches nothing: a count of 0, not an error.
 * PSS_EINVAL (message in pss_last_error, *out / counts untouched): an empty pattern (as an empty term is), offsets that do not
 * start at 0 or that decrease, a null qbytes / qoffsets with nq > 0, a null out / counts, patterns whose expansion (below)
 * holds more than the 2^32 - 1 terms an all-terms batch takes, a pattern of more than 2^32 - 1 bytes (a chunk has fewer), a
 * null reader (judged last, as for the all-terms calls).
 * The search: the suffix arrays are exact-byte, so the host expands.  The SEED of a pattern is its longest window that holds
 * at most F = PSS_ICASE_SEED_LETTERS ASCII letters (1 .. 6, default 5), the leftmost on a tie; bytes that are no letters cost
 * nothing (`user_id=12345678` seeds with `ser_id=12345678`).  The 2^f spellings of the seed (f <= F its letter count), in
 * ASCENDING byte order -- upper case before lower, the first letter most significant -- are the terms of one group of an
 * all-terms-shaped batch; the interval search answers every (spelling, chunk) pair, and the hits of a (pattern, chunk) pair
 * are its spellings' intervals one behind the other: disjoint and ascending, so still in suffix-array order.  Every hit is
 * verified on the device: the whole pattern around the seed occurrence under fold, then the entry in front of the match for
 * an earlier folded occurrence -- the hit of an entry's LEFTMOST folded match stands for the entry, whatever mix of spellings
 * the entry holds.  The answer is exact for every pattern length.  pss_icase_variants shows the expansion.  It is the
 * one-term case of pss_reader_search_terms_icase_batch: every pattern a group of one include term.
 * Order: pattern-major, chunk-major inside a pattern; inside one (pattern, chunk) pair the suffix-array order of the seed's
 * occurrence inside each entry's leftmost folded match, the same for the text and the id variant -- pss_reader_set_result_order
 * has no effect.  A pattern without an ASCII letter returns exactly what pss_reader_search_ids_batch returns for it under the
 * default order, order included.
 * Whole-file, sharded and multi-device readers, and suffix arrays on the host tier, are served alike.
 * pss_reader_last_stats: queries = patterns, hits = the sum of the spellings' interval hits -- the candidates --, entries =
 * what is returned; route = GENERAL | the interval bits (| COUNTS for the count call) -- there is no bit of its own.  The id
 * variant builds the line tables on first use, the other two allocate nothing for them.
 * The limit: the candidates follow the occurrences of the folded SEED, not of the pattern -- a long pattern whose seed is a
 * common word looks at every occurrence of that word.
 * Out of scope: folding outside ASCII; a case-insensitive anchored call of its own (the all-terms and the wildcard search under
 * fold are the calls further down; "starts with / ends with / equals" under fold is the wildcard call's `p*`, `*p`, `p`); the
 * fused, resident and mid paths (a case-insensitive batch always takes the general pipeline); a device-resident result; the multi-process gather over
 * RCCL (dist.ShardedReader); walking only the spellings that are PRESENT, on the device (the blind enumeration probes up to
 * 2^F mostly empty intervals per pattern and chunk: the price of reusing the interval kernels as they are); picking the rarer
 * of two seeds per chunk.
 */
/* packed entry text, one row per pattern */
int pss_reader_search_icase_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_icase_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, pss_result **out);
/* counts[q] = entries pattern q matches; nothing but nq counters comes down */
int pss_reader_count_icase_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, uint64_t *counts);
/* The expansion of ONE pattern, on the host: no reader, no GPU.  letters = the letters of the seed at most, 1 .. 6; <= 0 means
 * the configured value (PSS_ICASE_SEED_LETTERS).  *seed_off / *seed_len = the seed's window inside the pattern, *count = its
 * 2^f spellings; out (cap bytes, or NULL for the sizes alone) receives them back to back, *seed_len bytes each, ascending.
 * PSS_EINVAL: an empty pattern, letters > 6, a null seed_off / seed_len / count, cap < *count * *seed_len. */
int pss_icase_variants(const uint8_t *pat, uint64_t len, int32_t letters, uint8_t *out, uint64_t cap, uint32_t *seed_off,
                       uint32_t *seed_len, uint32_t *count);
/*
 * Case-insensitive all-terms and wildcard search (no reference counterpart): pss_reader_search_terms_batch and
 * pss_reader_search_seq_batch under the fold of pss_reader_search_icase_batch.  Arguments exactly as their exact-byte
 * namesakes take them.  Fold is ASCII only: A .. Z are equivalent to a .. z, every other byte, 0x80 .. 0xFF included, equals
 * only itself.  An entry is the bytes [start, end) of a chunk's text, end = its closing 0x0A or the length n of the text.
 *   All-terms under fold: group (include, exclude) matches an entry iff every include term occurs in it under fold and no
 *   exclude term does.  An include term holding 0x0A voids its group (count 0, no hit looked at); an exclude term holding 0x0A
 *   is ignored.
 *   Wildcard under fold: the segment / anchor semantics of pss_reader_search_seq_batch -- segments in order, without overlap,
 *   leftmost-greedy; START / END pin the first / last segment to the entry's ends -- with every byte comparison under fold.
 *   `a*A` does not match the entry `a`; `ab*BA` matches `abBA` and not `aBa`; one segment with both anchors is "the entry equals
 *   it under fold".  So case-insensitive "starts with / ends with / equals" are the groups (p, START), (p, END), (p, START | END).
 * PSS_EINVAL (message in pss_last_error naming the term or segment and the group, *out / counts untouched): whatever the
 * exact-byte namesake refuses (an empty term or segment, a group without an include term or without a segment, bad flags,
 * anchors or offsets, null arguments, a null reader judged last), a term of more than 2^32 - 1 bytes, and a batch whose terms
 * expand to more than 2^32 - 1 spellings in all -- refused before anything is allocated for the expansion.
 * The search: the host expands every term (segment) as pss_reader_search_icase_batch expands a pattern -- its SEED under
 * PSS_ICASE_SEED_LETTERS, the seed's at most 64 spellings in ascending order, the term folded to lower case.  Three pair spaces
 * follow: the interval search answers every (spelling, chunk) pair; the counts of a term's spellings add up to the term's SEED
 * HITS per chunk; per (group, chunk) pair the include term (segment) with the fewest seed hits, the lowest index on a tie,
 * DRIVES.  The driver is chosen by seed occurrences -- which is what bounds the work -- not by occurrences of the term.  Every
 * seed hit of the driver is verified against the whole driver term under fold and deduplicated to the entry's leftmost folded
 * match, exactly as for pss_reader_search_icase_batch; each candidate entry is then scanned once, under fold, for the group's
 * other terms (an exclude term whose seed is absent from the chunk is not looked for), or walked once for the segments in order.
 * A chunk in which an include term's seed is absent contributes nothing without a hit being looked at.
 * Order: group-major, chunk-major inside a group; inside one (group, chunk) pair the suffix-array order of the driver term's
 * seed occurrence inside each entry's leftmost folded match of the driver term; the same for the text and the id variant --
 * pss_reader_set_result_order has no effect.  A group without an ASCII letter returns exactly what the exact-byte call
 * returns; a group of one include term and no exclude term, and the pattern `*p*`, return exactly what
 * pss_reader_search_icase_ids_batch returns for the term.
 * Whole-file, sharded and multi-device readers, and suffix arrays on the host tier, are served alike.
 * pss_reader_last_stats: queries = groups, hits = the sum over the (group, chunk) pairs of the driver term's seed hits,
 * entries = what is returned; route = GENERAL | the interval bits (| COUNTS for the count calls) -- no bit of its own.
 * Out of scope: folding outside ASCII; a case-insensitive route through the anchored search's "\n" + s intervals; the fused,
 * mid, resident and device-resident paths; the multi-process gather over RCCL (dist.ShardedReader); probing only the spellings
 * that are present; choosing the driver by anything finer than seed hits; `?` and character classes.
 */
/* packed entry text, one row per group */
int pss_reader_search_terms_icase_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms,
                                        const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *exclude, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_terms_icase_ids_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms,
                                            const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *exclude, pss_result **out);
/* counts[g] = entries group g matches; nothing but ngroups counters comes down */
int pss_reader_count_terms_icase_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms,
                                       const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *exclude, uint64_t *counts);
/* packed entry text, one row per group */
int pss_reader_search_seq_icase_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs,
                                      const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_seq_icase_ids_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs,
                                          const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, pss_result **out);
/* counts[g] = entries group g matches; nothing but ngroups counters comes down */
int pss_reader_count_seq_icase_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs,
                                     const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, uint64_t *counts);
/*
 * Search within k mismatches (no reference counterpart): per pattern, the entries that hold it with at most k bytes
 * SUBSTITUTED -- Hamming distance, `passw0rd` for `password` at k = 1.  Arguments as pss_reader_search_batch takes them, plus k:
 * nq budgets, one per pattern, each 0 .. 3.
 * Entry [start, end) is the bytes of a chunk's text up to the closing 0x0A, or up to the length n of the text for an
 * unterminated last entry (whose last byte takes part, as in the case-insensitive search).  The entry matches pattern p within k
 * mismatches iff some m in start .. end - |p| has at most k indices i with text[m + i] != p[i].  The window lies INSIDE THE
 * ENTRY: a window that reaches over a newline is no match, even when the newline is one of its at most k differing bytes.
 * Bytes are exact: nothing folds, and 0x80 .. 0xFF and 0x00 are bytes like any other.  One row per pattern, packed as
 * pss_reader_search_batch (text) and pss_reader_search_ids_batch (ids) pack theirs; every entry at most once per pattern.  A
 * pattern that holds 0x0A counts 0 and no hit is looked at.  k = 0 returns exactly what pss_reader_search_ids_batch returns for
 * the pattern under the default order: the same ids in the same order.
 * PSS_EINVAL (message in pss_last_error, *out / counts untouched): an empty pattern; a pattern of at most k bytes (every window
 * would match it: the question is about entry lengths, not content); k > 3; offsets that do not start at 0 or that decrease; a
 * null qbytes / qoffsets / k with nq > 0; a null out / counts; a pattern of more than 2^32 - 1 bytes; a null reader (judged
 * last: a malformed batch is reported as such with or without one).
 * The search: pigeonhole seeds and a verify step.  The host cuts pattern p of L bytes into k + 1 PIECES, piece j =
 * p[j L / (k + 1), (j + 1) L / (k + 1)) in integer division -- non-empty because L > k; pss_near_pieces shows them.  k
 * mismatches cannot touch all k + 1 pieces, so every window within budget holds at least one piece exactly, at its offset.  The
 * pieces are the queries of the interval search; every hit of every piece is verified on the device: the window it implies must
 * lie inside the chunk and inside the hit's entry, differ from the pattern in at most k bytes, and the piece must be the FIRST
 * exact piece of that window (a window that holds two pieces exactly is one candidate, not two); then the entry in front of the
 * window is scanned for an earlier window within budget -- the hit of the entry's LEFTMOST near match stands for the entry.
 * Pieces may repeat (`abab`, k = 1) or nest, so a (pattern, chunk) pair's candidates are the plain sum of its pieces' interval
 * hits, up to (k + 1) n; a pair whose sum passes 2^32 - 1 fails the batch with PSS_EINVAL before any hit is looked at.
 * Order: pattern-major, chunk-major inside a pattern; inside one (pattern, chunk) pair by the index of the first exact piece of
 * each entry's leftmost near match, and inside one piece by the suffix-array order of the suffix at that piece's occurrence; the
 * same for the text and the id variant -- pss_reader_set_result_order has no effect.
 * Whole-file, sharded and multi-device readers, and suffix arrays on the host tier, are served alike.
 * pss_reader_last_stats: queries = patterns, hits = the sum over pieces and chunks of the piece's exact occurrences -- the
 * candidates --, entries = what is returned; route = GENERAL | the interval bits (| COUNTS for the count call) -- there is no
 * bit of its own.  The id variant builds the line tables on first use, the other two allocate nothing for them.
 * The limit: the candidates follow the occurrences of the PIECES -- a short pattern at k = 3 has pieces of a byte or two, and
 * every occurrence of such a piece is verified.
 * Out of scope: insertions and deletions (the search within k edits below has them); k > 3; mismatches inside all-terms groups
 * or wildcard patterns (under ASCII case folding: pss_reader_search_near_icase_batch below); the fused, mid, resident and device-resident paths (a near batch always takes the general pipeline); the
 * multi-process gather over RCCL (dist.ShardedReader); choosing pieces by rarity; a piece driving only where it is present.
 */
/* packed entry text, one row per pattern; k = nq budgets */
int pss_reader_search_near_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                 pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_near_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                     pss_result **out);
/* counts[q] = entries pattern q matches within k[q] mismatches; nothing but nq counters comes down */
int pss_reader_count_near_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                uint64_t *counts);
/* The expansion of ONE pattern, on the host: no reader, no GPU.  offsets / lengths (room for k + 1 values each) receive the
 * pieces' windows inside the pattern, left to right, *count = k + 1.
 * PSS_EINVAL: an empty pattern, k > 3, len <= k, len > 2^32 - 1, a null offsets / lengths / count. */
int pss_near_pieces(const uint8_t *pat, uint64_t len, uint32_t k, uint32_t *offsets, uint32_t *lengths, uint32_t *count);
/*
 * Search within k edits (no reference counterpart): per pattern, the entries that hold it with at most k bytes INSERTED,
 * DELETED or SUBSTITUTED -- Levenshtein distance over bytes: `pasword`, `passsword` and `passw0rd` for `password` at k = 1.
 * Arguments, packing, the ids variant and the count call as for the search within k mismatches above; k is nq budgets, 0 .. 3.
 * An entry with true bytes e -- text[start, newline), or text[start, n) for an unterminated last entry -- matches pattern p
 * within k edits iff some substring w of e has lev(w, p) <= k, where an insertion, a deletion and a substitution of a single
 * BYTE cost 1 each.  w lies inside the entry because e holds no newline: a match never reaches over a newline, even where
 * "delete the newline" would be one of its edits.  Bytes are exact: nothing folds, and 0x00 and 0x80 .. 0xFF are bytes like
 * any other.  Every entry at most once per pattern.  A pattern that holds 0x0A matches nothing and no hit is looked at (near's
 * rule, kept so that the two calls agree).  k = 0 returns exactly what pss_reader_search_ids_batch returns, order included; for
 * every k the answer contains, as a set, what pss_reader_search_near_ids_batch returns at the same k.
 * PSS_EINVAL (message in pss_last_error, *out / counts untouched): an empty pattern; a pattern of at most k bytes (deleting all
 * of it would match every entry); k > 3; and every malformed batch the near calls name, with or without a reader (the reader is
 * judged last).
 * The search: near's pieces (pss_near_pieces serves both kinds), the same seed queries at the same positions.  k edits cannot
 * touch all k + 1 pieces, so every w within budget holds some piece j exactly -- but, unlike under mismatches, not at a known
 * offset inside w.  A CANDIDATE is (piece j, exact occurrence at text offset d); with off_j / len_j the piece's window in p it
 * STANDS iff lc + rc <= k, where
 *   lc = the least lev(text[a, d), p[0, off_j)) over a in [entry start, d] and
 *   rc = the least lev(text[d + len_j, b), p[off_j + len_j, L)) over b in [d + len_j, entry end];
 * the two sides are independent, the left computed within k and the right within k - lc, each as a banded DP of at most 7 cells a
 * row that stops at a newline, at 0 and at n.  An entry matches iff one of its candidates stands.  The ONE hit kept per entry is
 * the standing candidate with the smallest d and, among equal d (two pieces are exact at one d only when one is a prefix of the
 * other, as `aab` + `aa`), the smallest j: a hit is dropped when an earlier piece stands at its d, and the entry in front of d is
 * scanned for a standing candidate.
 * Order: pattern-major, chunk-major inside a pattern; inside one (pattern, chunk) pair by the piece index j of each entry's kept
 * candidate, and inside one piece by the suffix-array order of the suffix at d; the same for text and ids --
 * pss_reader_set_result_order has no effect.  Whole-file, sharded and multi-device readers, and suffix arrays on the host tier,
 * are served alike.
 * pss_reader_last_stats: as for the near calls -- hits = the sum over pieces and chunks of the pieces' exact occurrences,
 * entries = what is returned, route = GENERAL | the interval bits (| COUNTS); no bit of its own.
 * The limits: near's (every occurrence of every piece is verified), and an entry DENSE with occurrences of a piece: the scan
 * in front of a hit runs both DPs at every such occurrence, lane by lane.
 * Out of scope: edits inside all-terms groups or wildcard patterns (under ASCII case folding:
 * pss_reader_search_near_icase_batch below); k > 3; a transposition as one
 * edit; the fused, mid, resident and device-resident paths; choosing pieces by rarity.
 */
/* packed entry text, one row per pattern; k = nq budgets */
int pss_reader_search_edit_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                 pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_edit_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                     pss_result **out);
/* counts[q] = entries pattern q matches within k[q] edits; nothing but nq counters comes down */
int pss_reader_count_edit_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                uint64_t *counts);
/*
 * Search within k mismatches or k edits UNDER ASCII CASE FOLDING (no reference counterpart): the two searches above with one
 * other rule of equality -- two bytes are equal iff they are equal after folding A-Z to a-z, the rule of
 * pss_reader_search_icase_batch.  Nothing else folds: `@` and '`', `[` and `{`, 0xC9 and 0xE9 are different bytes, and 0x00 and
 * 0x80 .. 0xFF match only themselves.  `passw0rd` and `PASSW0RD` are both found for `Password` at k = 1: a case difference costs
 * nothing.  Arguments, packing, the ids variant and the count call as for the near calls, plus `edits`: 0 counts substituted bytes
 * (an entry matches iff some window of |p| bytes inside it differs from p in at most k positions under that equality), anything
 * else counts edits (iff some substring of the entry has Levenshtein distance <= k to p, a substitution of fold-equal bytes
 * costing 0).  The window or substring lies inside the entry.  k is nq budgets, 0 .. 3.  A pattern that holds 0x0A matches
 * nothing and no hit is looked at; every entry at most once per pattern.  k = 0 returns exactly what
 * pss_reader_search_icase_ids_batch returns, order included; for every k the answer contains the exact-byte answer at the same
 * k, and the edits answer contains the mismatch answer.
 * PSS_EINVAL: what the near and edit calls name, in the same order; the reader is judged last.
 * The search: the pattern folded to lower case is the term that is verified; its pieces are near's (pss_near_pieces); each piece
 * is looked up as a case-insensitive term is, through the spellings of its SEED -- the longest window of the piece with at most f
 * ASCII letters, leftmost on a tie, f = min(PSS_ICASE_SEED_LETTERS, cap(k)) with cap = 6, 5, 4, 4 for k = 0 .. 3: the largest f
 * with (k + 1) 2^f <= 64, so a pattern has at most 64 seed queries.  pss_near_seeds shows them.  Every hit of every query is
 * verified on the device under fold: its piece must be fold-equal over its whole length where the seed puts it; under
 * mismatches the window must be within budget inside the hit's entry and the piece its first fold-exact one, and no window
 * within budget may start in front of it in the entry; under edits the candidate (piece, position) must stand, no earlier piece
 * may stand at the same position, and no candidate may stand in front of it in the entry.
 * Order: pattern-major, chunk-major inside a pattern; inside one pair by the piece index of the kept hit, then by query (the
 * spellings ascend bytewise), then in suffix-array order; pss_reader_set_result_order has no effect.  Always the general pipeline.
 * pss_reader_last_stats: hits = the sum over all seed queries and chunks of their exact occurrences, entries = what is returned.
 * Out of scope: folding outside ASCII; budgets under fold inside all-terms groups or wildcard patterns; choosing pieces by rarity.
 */
/* packed entry text, one row per pattern; k = nq budgets; edits: 0 = mismatches, else edits */
int pss_reader_search_near_icase_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                       int edits, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_near_icase_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                           const uint8_t *k, int edits, pss_result **out);
/* counts[q] = entries pattern q matches within k[q] under fold; nothing but nq counters comes down */
int pss_reader_count_near_icase_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                      int edits, uint64_t *counts);
/* The seed queries of ONE pattern under fold, on the host: no reader, no GPU.  piece / pos / lengths (room for 64 values each)
 * receive per query, in the order of the search, the index of its piece, its position inside the pattern and its length;
 * *count = the number of queries (at most 64).  out (cap bytes; null: the sizes alone) receives the queries' bytes back to back.
 * letters: 1 .. 6, or <= 0 for the configured PSS_ICASE_SEED_LETTERS; the cap of k bounds it.
 * PSS_EINVAL: an empty pattern, k > 3, len <= k, letters > 6, len > 2^32 - 1, a null piece / pos / lengths / count, an out
 * too small (*count is set). */
int pss_near_seeds(const uint8_t *pat, uint64_t len, uint32_t k, int32_t letters, uint8_t *out, uint64_t cap, uint32_t *piece,
                   uint32_t *pos, uint32_t *lengths, uint32_t *count);
/*
 * ANY-OF search (no reference counterpart): `grep -e error -e warn -e fatal` over the entries -- per SET of alternatives the
 * entries that contain at least one of them.  An entry is the bytes [start, end) of a chunk's text as the all-terms search takes
 * them, the last byte of an unterminated last entry included.  Bytes are exact; under PSS_ANY_ICASE the rule is
 * pss_reader_search_icase_batch's: A-Z and a-z fold and nothing else does.  Every entry comes at most once per set.
 * Arguments: nalts alternatives back to back in abytes, cut by aoffsets (nalts + 1); set g is the alternatives set_offsets[g] ..
 * set_offsets[g + 1] (nsets + 1 offsets, the last = nalts).  One row per set, packed as pss_reader_search_terms_batch packs its
 * groups; flags is 0 or PSS_ANY_ICASE.
 * Normalisation (host only, csrc/any_terms.h; pss_any_alternatives shows its result), in this order: under PSS_ANY_ICASE every
 * alternative is folded to lower case; duplicates go; an alternative that holds 0x0A goes -- it occurs in no entry, and it
 * voids itself, not its set --; an alternative that holds another one as a substring goes (it asks nothing more of an entry);
 * the rest is sorted ascending bytewise.  What is left is prefix-free: no two alternatives can start at one text position.  A
 * set whose alternatives all held 0x0A matches nothing: a count of 0, not an error.
 * The search: a set is ONE term of a seeded batch (the case-insensitive and the near searches are the others), its alternatives
 * back to back.  Exact: every alternative is one query at position 0.  Under PSS_ANY_ICASE every alternative is looked up through
 * the spellings of its SEED, the longest window with at most F ASCII letters, leftmost on a tie, F = min(PSS_ICASE_SEED_LETTERS,
 * floor(log2(64 / alternatives))): a set keeps the at most 64 queries the seeded kernels are written for, and F >= 1 is what caps
 * a set at PSS_ANY_MAX_ALTS_ICASE.  Every hit is verified on the device (under fold its alternative over its whole length where
 * the seed puts it) and kept iff no alternative of the set starts in front of it in its entry: the entry's leftmost match.
 * Order: set-major, chunk-major inside a set, inside one pair the set's queries one interval behind the other -- exact: by
 * alternative (ascending), then in suffix-array order, which for a normalised set IS suffix-array order of each entry's leftmost
 * match of any alternative, so a set of one alternative returns what pss_reader_search_ids_batch returns under the default order;
 * under fold: by alternative, then spelling (ascending), then suffix-array order of the seed occurrence, so a set of one
 * alternative returns what pss_reader_search_icase_ids_batch returns.  pss_reader_set_result_order has no effect.  Always the
 * general pipeline, no route bit of its own.  pss_reader_last_stats: hits = the sum over all queries and chunks of their exact
 * occurrences, entries = what is returned.
 * PSS_EINVAL (message in pss_last_error, *out / counts untouched), in this order: a null out / counts; a null abytes / aoffsets
 * with nalts > 0 or a null set_offsets with nsets > 0; flags other than PSS_ANY_ICASE; alternative offsets that do not start at
 * 0 or that decrease, set offsets that do not start at 0, that decrease or that do not end at nalts; then the first bad set as
 * "set <g>: ...": a set without an alternative, an empty alternative, one of more than 2^32 - 1 bytes, more than
 * PSS_ANY_MAX_ALTS alternatives after normalisation (PSS_ANY_MAX_ALTS_ICASE under PSS_ANY_ICASE); a null reader last.  Nothing
 * is launched before all of that has passed.
 * Not built: any-of clauses inside all-terms groups or wildcard patterns; an alternation driving pss_reader_search_regex_batch
 * (it would hand this path its required set); budgets on alternatives; spans of alternatives; the fused, resident and mid
 * paths, a device-resident result, dist.ShardedReader; a one-pass multi-pattern scan (Aho-Corasick, a first-byte bitmap);
 * seed letters budgeted per alternative.
 */
#define PSS_ANY_ICASE 1u
#define PSS_ANY_MAX_ALTS 64u
#define PSS_ANY_MAX_ALTS_ICASE 32u
/* packed entry text, one row per set */
int pss_reader_search_any_batch(pss_reader *r, const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts,
                                const uint64_t *set_offsets, uint32_t nsets, uint32_t flags, pss_result **out);
/* u64 entry ids, packed as pss_reader_search_ids_batch packs them */
int pss_reader_search_any_ids_batch(pss_reader *r, const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts,
                                    const uint64_t *set_offsets, uint32_t nsets, uint32_t flags, pss_result **out);
/* counts[g] = entries set g matches; nothing but nsets counters comes down */
int pss_reader_count_any_batch(pss_reader *r, const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts,
                               const uint64_t *set_offsets, uint32_t nsets, uint32_t flags, uint64_t *counts);
/* ONE set normalised, on the host: no reader, no GPU.  out (cap bytes: aoffsets[nalts] always suffice) receives the alternatives
 * left back to back, offsets (room for nalts + 1) their *count + 1 offsets, seed_pos / seed_len (room for nalts each) per
 * alternative the position and length of what is looked up inside it: 0 and its length, or under PSS_ANY_ICASE its seed
 * (pss_icase_variants of those bytes with the set's F gives the queries).  letters: 1 .. 6, or <= 0 for the configured
 * PSS_ICASE_SEED_LETTERS; the set's size bounds it.
 * PSS_EINVAL: a null out / offsets / seed_pos / seed_len / count, letters > 6, then what the calls above name for one set. */
int pss_any_alternatives(const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts, uint32_t flags, int32_t letters,
                         uint8_t *out, uint64_t cap, uint64_t *offsets, uint32_t *seed_pos, uint32_t *seed_len, uint32_t *count);
/*
 * MATCH SPANS (no reference counterpart): where in an entry a pattern's best match stands, how long it is and how close, for
 * rows of (entry id, pattern) -- the third call beside "which entries" (the *_ids_batch calls) and "their text"
 * (pss_reader_entries_by_id).  12 bytes per row come down; no text does.
 * Rows id_offsets[q] .. id_offsets[q + 1] of `ids` belong to pattern q (bytes qbytes[qoffsets[q], qoffsets[q + 1]), budget k[q]
 * = 0 .. 3); out[i] answers ids[i], in the order given.  Repeated ids, and ids of several chunks in any order, are fine.
 * flags: PSS_SPAN_EDITS -- the budget counts edits, not substituted bytes; PSS_SPAN_ICASE -- bytes are equal as in
 * pss_reader_search_near_icase_batch (after folding A-Z to a-z, nothing else), else exactly.
 * Let e be the entry's true bytes (text[start, newline), or text[start, n) for an unterminated last entry) and p the pattern.  A
 * candidate is a substring e[s, s + l): without EDITS l = |p| and its distance d is the number of differing bytes; with EDITS
 * any l >= 1 and d = lev(e[s, s + l), p) over bytes.  It counts only if d <= k, and it lies inside the entry by construction
 * (e holds no newline).  The row's answer is the candidate with the least (d, s, -l): closest first, then leftmost, then
 * longest -- {start = s, length = l, distance = d}, offsets in BYTES from the entry's first byte.  A row with no candidate is
 * {-1, 0, -1}: a legal row, not an error, since ids may come from anywhere.  A pattern that holds 0x0A gives {-1, 0, -1} in all
 * its rows (the search calls' rule).  Hence distance >= 0 exactly for the ids pss_reader_search_near_ids_batch /
 * _edit_ids_batch / _near_icase_ids_batch return for the same pattern and budget, and without EDITS length == |p|.
 * "Closest first" is deliberate: the search keeps an entry's LEFTMOST match within budget, but `passw0rd` is not what to
 * highlight in a line that also holds `password`.
 * PSS_EINVAL (message in pss_last_error, out untouched), judged before the reader is looked at and before anything is launched,
 * as the near calls do: an empty pattern; a pattern of at most k bytes; k > 3; unknown flag bits; id_offsets that do not ascend
 * from 0; null pointers where rows or patterns exist.  Then, with pss_reader_entries_by_id's message: an id of a chunk this
 * reader does not hold, or a line past the chunk's last entry.  nq = 0, or zero rows, is PSS_OK and writes nothing.
 * A multi-device reader splits the rows by part and puts the answers back in the order asked; a sharded reader answers for the
 * chunks it holds.  The scan: one wavefront per row, 64 start positions a step; one wait on the stream.
 * pss_reader_last_stats is left as it was.
 * Out of scope: spans of wildcard pieces and of all-terms groups (call once per term); more than one span per entry; spans
 * straight out of the search calls.
 */
typedef struct pss_span { int32_t start, length, distance; } pss_span;
#define PSS_SPAN_EDITS 1u
#define PSS_SPAN_ICASE 2u
int pss_reader_match_spans(pss_reader *r, const uint64_t *ids, const uint64_t *id_offsets /* nq + 1 */, const uint8_t *qbytes,
                           const uint64_t *qoffsets, uint32_t nq, const uint8_t *k, uint32_t flags,
                           pss_span *out /* id_offsets[nq] rows, the caller's */);
/* For the first `cap` resident chunks, in file order: index in the file and number of entries; *num = resident chunks. */
int pss_reader_chunk_entries(pss_reader *r, uint64_t *chunk_index, uint64_t *entries, uint64_t cap, uint64_t *num);
/*
 * The same search with the packed result LEFT ON THE DEVICE: the multi-GPU gather (RCCL send / recv of
 * device buffers to the collecting rank, pysubstringsearch_amd/dist.py) takes it from there, so a
 * contributing rank never moves an entry through its host.  Replaces, across GPUs, what
 * `results.lock().extend(local_results)` does across chunk threads in src/lib.rs:280-284.  The pointers
 * are workspace of the device context: valid until the next search or build on that device.
 */
typedef struct pss_device_result {
    uint64_t num_queries;
    uint64_t num_entries;
    uint64_t num_bytes;
    const void *d_counts;    /* u64 [num_queries]  entries per query */
    const void *d_offsets;   /* u64 [num_entries]  start of every entry in d_bytes (entry e ends where e + 1 starts,
                                the last one at num_bytes) */
    const void *d_bytes;     /* u8  [num_bytes]    entries back to back, query-major, chunk-major inside a query */
    int32_t device;
} pss_device_result;
int pss_reader_search_batch_device(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets,
                                   uint32_t nq, pss_device_result *out);
/*
 * Gather of per-rank packed results over RCCL, torch-free (one process per GPU; src/lib.rs:205-207, 280-284 is what it
 * replaces: rayon tasks appending to one Vec under a mutex).  pss_comm_unique_id: 128 bytes (an ncclUniqueId) made by ONE
 * rank and shipped to the others by any means; pss_comm_init: every rank, same id, its rank and its device (collective).
 * pss_gather_packed_rccl: every rank of the communicator calls it with the pss_device_result of ITS chunks for the same
 * queries (pss_reader_search_batch_device); rank dst receives the others' buffers device to device (one grouped
 * ncclSend / ncclRecv batch), merges on its GPU (query-major, rank-major inside a query) and gets the packed result in
 * *out (pss_result_*); the other ranks get *out = NULL.  The RCCL entry points are looked up at run time in the librccl
 * the process has loaded (PSS_RCCL_LIB names another): libpss.so does not link it.
 */
typedef struct pss_comm pss_comm;
int pss_comm_unique_id(uint8_t *id128);
int pss_comm_init(const uint8_t *id128, int32_t world, int32_t rank, int32_t device, pss_comm **out);
int pss_comm_destroy(pss_comm *c);
int pss_gather_packed_rccl(pss_comm *c, const pss_device_result *mine, int32_t dst, pss_result **out);
/*
 * Failure behaviour of the gather (round 5).  Every wait for the peers is bounded: PSS_RCCL_TIMEOUT_MS in the
 * environment (default 60000), pss_comm_set_timeout_ms per communicator; RCCL's asynchronous error state is polled
 * meanwhile.  When the bound passes, or RCCL reports an error, the communicator is ABORTED (ncclCommAbort), the call
 * returns PSS_EDEVICE with the reason in pss_last_error, and every later call on that communicator returns PSS_EDEVICE
 * at once -- readers, builders and other communicators of the process keep working; make a new communicator to go on.
 * The outcome is collective where it can be: a rank that cannot go through with the exchange (the collecting rank out
 * of memory, ranks that answered different numbers of queries) says so in a go / no-go word before anybody sends, and
 * every rank returns an error.  No device context is held while the call waits for a peer.
 * pss_comm_status: PSS_OK while the communicator is usable, PSS_EDEVICE once it was aborted; counters of completed
 * gathers and of aborts (either pointer may be NULL).
 */
int pss_comm_set_timeout_ms(pss_comm *c, uint32_t ms);
int pss_comm_status(pss_comm *c, uint64_t *gathers, uint64_t *aborts);
/*
 * The collectives library as a table (round 5).  By default libpss looks RCCL up in the process (dlopen of librccl.so,
 * PSS_RCCL_LIB).  An application that links RCCL itself hands its entry points in -- signatures as in rccl.h, streams
 * and communicators as void pointers -- and may adopt a communicator it already has (pss_comm_adopt: never destroyed
 * by pss_comm_destroy, but aborted when a gather times out).  The test-suite uses the same seam to make Send / Recv /
 * GroupEnd fail and a Recv never complete.  comm_abort, comm_get_async_error, get_error_string, get_unique_id,
 * comm_init_rank and comm_destroy may be NULL (the last three: pss_comm_adopt only).  NULL restores the lookup;
 * communicators keep the table they were made with.
 */
typedef struct pss_rccl_unique_id { char internal[128]; } pss_rccl_unique_id;      /* ncclUniqueId */
typedef struct pss_rccl_api {
    int (*get_unique_id)(pss_rccl_unique_id *id);
    int (*comm_init_rank)(void **comm, int nranks, pss_rccl_unique_id id, int rank);
    int (*comm_destroy)(void *comm);
    int (*comm_abort)(void *comm);
    int (*comm_get_async_error)(void *comm, int *async_error);
    int (*group_start)(void);
    int (*group_end)(void);
    int (*send)(const void *buf, size_t count, int datatype, int peer, void *comm, void *stream);
    int (*recv)(void *buf, size_t count, int datatype, int peer, void *comm, void *stream);
    int (*all_gather)(const void *sendbuf, void *recvbuf, size_t sendcount, int datatype, void *comm, void *stream);
    const char *(*get_error_string)(int result);
} pss_rccl_api;
int pss_rccl_inject(const pss_rccl_api *api);
int pss_comm_adopt(void *nccl_comm, int32_t world, int32_t rank, int32_t device, pss_comm **out);

/*
 * Host merge of `world` packed results of the same nq queries (one per rank, each query-major) into one:
 * query-major, rank-major inside a query -- the cross-chunk concatenation of src/lib.rs:280-286 across
 * ranks.  counts[r] = u64[nq], offsets[r] = u64[num_entries[r]] entry starts, bytes[r] = num_bytes[r]
 * bytes.  out_counts[nq], out_offsets[sum(num_entries) + 1], out_bytes[sum(num_bytes)] are the caller's.
 */
int pss_merge_packed(uint32_t world, uint64_t nq, const uint64_t *const *counts, const uint64_t *const *offsets,
                     const uint8_t *const *bytes, const uint64_t *num_entries, const uint64_t *num_bytes,
                     uint64_t *out_counts, uint64_t *out_offsets, uint8_t *out_bytes);
/* The same merge with every buffer resident in the HBM of `device` (the collecting rank of a multi-GPU gather holds
 * its own result and the ones RCCL delivered there): one merged result to bring down instead of `world`.
 * d_starts[r] = u64[num_entries[r]] entry starts (pss_device_result.d_offsets); d_out_offsets receives
 * sum(num_entries) + 1 entries, d_out_counts nq, d_out_bytes sum(num_bytes).  world <= 16. */
int pss_merge_packed_device(int32_t device, uint32_t world, uint64_t nq, const void *const *d_counts,
                            const void *const *d_starts, const void *const *d_bytes, const uint64_t *num_entries,
                            const uint64_t *num_bytes, void *d_out_counts, void *d_out_offsets, void *d_out_bytes);
int pss_reader_last_stats(const pss_reader *r, pss_search_stats *stats);
/* Drops the chunks and closes the reader. */
int pss_reader_close(pss_reader *r);

/* Result accessors; memory stays owned by the result until pss_result_free. */
uint64_t pss_result_num_queries(const pss_result *res);
uint64_t pss_result_num_entries(const pss_result *res);
const uint64_t *pss_result_query_counts(const pss_result *res);  /* [num_queries] entries per query */
const uint64_t *pss_result_offsets(const pss_result *res);       /* [num_entries + 1] into bytes */
const uint8_t *pss_result_bytes(const pss_result *res);
void pss_result_free(pss_result *res);

/* ---- synthetic corpora (used by bench.py and the tests) -- */

#define PSS_CORPUS_LINES 0     /* 38-symbol alphabet, '\n' with p = 1/40 */
#define PSS_CORPUS_WORDS 1     /* 65536-word vocabulary, skewed, realistic LCP */
#define PSS_CORPUS_RUNS 2      /* lines of one repeated symbol from {a,b}, run <= 8192 */
#define PSS_CORPUS_PERIODIC 3  /* "a"*4095 + "\n" repeated */
#define PSS_CORPUS_REPEAT_LINE 4 /* one 40-byte line repeated (period 40, no runs of equal bytes) */
#define PSS_CORPUS_DUP_BLOCKS 5  /* a 1 MiB block of `lines` text repeated, 16 single-byte edits per copy */
#define PSS_CORPUS_MIXED 6       /* `words` whose middle third is one 60-byte line repeated, then 64 KiB blocks copied from the first third */
#define PSS_CORPUS_SOURCE 7      /* source-like text: 200-odd byte values, indentation, licence headers, stretches of lines copied from earlier in the chunk (round 5) */
/* Fills out[0..n) on the host; deterministic in (kind, n, chunk_index). */
int pss_gen_corpus(int kind, uint8_t *out, uint64_t n, uint64_t chunk_index);

#ifdef __cplusplus
}
#endif
#endif /* PSS_H */
