/*
 * snaphash.h -- C ABI of libsnaphash.so: the MI355X (gfx950) implementation of
 * snappy's per-file SHA-512 integrity pass (hashes.yaml).
 *
 * The reference (wolfbox/snappy 1.0.1, Go) has no FFI for this path; its seam
 * is two Go functions.  Each entry point below names the reference interface it
 * replaces (paths relative to the upstream tree):
 *
 *   helpers/helpers.go:187-201   func Sha512sum(infile string) (string, error)
 *   snappy/build.go:216-270      func writeHashes(buildDir, dataTar string) error
 *   snappy/hashes.go:25-110      yamlFileMode / fileHash / hashesYaml (format)
 *   snappy/click.go:330-338,970  writeHashesFile (install side: where Verify hooks in)
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ or torch types cross the line, and no
 *     C++ exception either: an allocation or thread-creation failure inside a call comes
 *     back as SNAPHASH_ENOMEM.
 *   - Return 0 on success, a negative SNAPHASH_E* code otherwise.  As in the
 *     reference (build.go:242-244) the first per-file error fails the whole
 *     batch and no output may be trusted.
 *   - There is no CPU fallback: without a usable gfx950 device snaphash_init fails with
 *     SNAPHASH_EDEVICE, and no error path re-routes a call.  Where a call's bytes are hashed is
 *     a planned decision (snaphash_config.host_threads): the HIP kernels take what many
 *     streams in parallel make fast, the library's own host SHA-512 (hostsha.cpp) takes what
 *     one SHA-512 stream at ~45 MB/s on the GPU would make slower than the reference's single
 *     goroutine; snaphash_stats_ex says which bytes went where, SNAPHASH_FLAG_GPU_ONLY keeps
 *     every byte on the GPU.
 *   - The caller owns every input and output buffer; the library keeps no caller
 *     pointer past return.  Only snaphash_tree's yaml_out and snaphash_walk's
 *     record set are library-allocated (snaphash_free / snaphash_records_free).
 *   - A ctx owns one or several devices (snaphash_config.devices) and is not
 *     thread-safe (one call in flight per ctx); distinct ctxs may be used
 *     concurrently.  With several devices the file list of a call is LPT-sharded
 *     inside the library (one host thread and one staging engine per device) and
 *     the digest vector is gathered with a single-process RCCL all-gather over
 *     xGMI.  No signal handlers are installed (the Go runtime owns them).
 *   - Process-wide effects: snaphash_init raises the soft RLIMIT_NOFILE to the hard limit (at most 65 536, as the Go
 *     runtime itself does at start-up) so that a hashing call can keep a file's descriptor open between the batches the
 *     file appears in (SNAPHASH_FLAG_KEEP_RLIMIT / SNAPHASH_KEEP_RLIMIT=1 leave it alone); the calling thread's memory
 *     policy and CPU affinity are left as they were found.
 *   - Digests are raw 64-byte big-endian SHA-512 values; the Go wrapper
 *     hex-encodes them with encoding/hex (lowercase, helpers.go:200).
 */
#ifndef SNAPHASH_H
#define SNAPHASH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNAPHASH_ABI_VERSION 5

enum {
    SNAPHASH_OK = 0,
    SNAPHASH_EINVAL = -1,   /* bad argument (NULL, misaligned device offset, ...) */
    SNAPHASH_ENOMEM = -2,   /* host or device allocation failed */
    SNAPHASH_EIO = -3,      /* open/read/lstat failed; errno in per-file status / last_error */
    SNAPHASH_EDEVICE = -4,  /* no gfx950 device, HIP error, kernel failure */
    SNAPHASH_EMODE = -5,    /* "Unknown file mode" (hashes.go:47): device, fifo, socket */
    SNAPHASH_ENAME = -6,    /* file name outside the plain-scalar set the YAML emitter reproduces */
    SNAPHASH_EPARSE = -7,   /* hashes.yaml text not understood */
    SNAPHASH_EMISMATCH = -8, /* snaphash_verify: tree differs from hashes.yaml */
    SNAPHASH_EFORMAT = -9,   /* not a valid gzip, DEFLATE, bzip2 or tar stream, or a CRC-32 / ISIZE mismatch */
    SNAPHASH_ECONTENT = -10  /* snaphash_tar_unpack(_bz2): a member name with "..", or a member type it does not unpack */
};

enum { /* snaphash_config.kernel */
    SNAPHASH_KERNEL_AUTO = 0, /* pick from the stream count and mean stream length */
    SNAPHASH_KERNEL_WIDE = 1, /* one lane per file stream does rounds + schedule (many-stream regime) */
    SNAPHASH_KERNEL_SPLIT = 2, /* rounds on one wave, message schedule on helper waves, K+W through
                                  an LDS ring (stream-starved regime: fewer streams than lanes) */
    SNAPHASH_KERNEL_PAIR = 3,  /* SPLIT with every stream carried by a lane pair (e-chain / a-chain,
                                  DPP exchange) */
    SNAPHASH_KERNEL_QUAD = 4   /* four lanes per stream (role x 32-bit half): fewest instructions on the critical wave */
};

typedef struct snaphash_ctx snaphash_ctx;

enum { /* snaphash_config.flags */
    SNAPHASH_FLAG_CHECK_GATHER = 1, /* several devices: also copy every device's digest slab to the host and
                                       require the RCCL-gathered vector to equal it (the collective's parity check) */
    SNAPHASH_FLAG_NO_RCCL = 2,      /* several devices: gather by per-device copies only */
    SNAPHASH_FLAG_FORCE_GATHER = 4, /* run the gather (RCCL with one rank) even on a single-device ctx: lets a
                                       1-GPU box exercise the collective path */
    /* ---- ABI 3 ---- */
    SNAPHASH_FLAG_GPU_ONLY = 8,     /* every byte of every stream is hashed by the HIP kernels, whatever it costs (the
                                       roofline runs and the parity tests of the kernels); host_threads is ignored */
    SNAPHASH_FLAG_NO_NUMA = 16,     /* do not place staging memory and fill threads on the GPU's NUMA node */
    /* ---- ABI 4 ---- */
    SNAPHASH_FLAG_KEEP_RLIMIT = 32, /* leave RLIMIT_NOFILE as it is (an application that select()s on descriptors must stay
                                       below FD_SETSIZE): files are then kept open between batches only within the soft
                                       limit found, the rest are opened segment by segment.  Also: SNAPHASH_KEEP_RLIMIT=1 */
    /* ---- ABI 5 ---- */
    SNAPHASH_FLAG_SPLIT_BLOCKS = 64 /* snaphash_gunzip_buffer / snaphash_tar_unpack: also cut a DEFLATE stream WITHOUT flush
                                       points (zlib's, Go's gzip.Writer: what click build, dpkg-deb and snappy build write)
                                       at its block boundaries, found by a GPU scan of every bit offset, and decode the
                                       blocks side by side (see snaphash_gunzip_buffer) */
};

typedef struct snaphash_config {
    uint32_t struct_size;   /* sizeof(snaphash_config); a caller built against ABI 1 passes the shorter size */
    int32_t device;         /* HIP device ordinal when n_devices == 0; -1 = the calling thread's current device */
    uint64_t staging_bytes; /* size of EACH of the two pinned-host/HBM staging buffers per device; 0 = 256 MiB */
    uint32_t kernel;        /* SNAPHASH_KERNEL_* */
    uint32_t deflate_depth; /* (ABI 4; was reserved, must be 0 before) the data.tar.gz producer's effort: hash-chain links the
                               DEFLATE search walks per position.  0 = 96 (since round 5; 32 before): the bytes of the
                               reference's gzip level 9 (clickdeb/deb.go:271) -- text 0.2392-0.2397 of the input against
                               zlib -9's 0.2394-0.2397, sources within 0.1 %, binaries under -- and still ahead of the one stream
                               that bounds the fused pass (the archive's SHA-512 on a host core).  32 = about zlib level 6's
                               output at 0.74x the kernel time, 72 = zlib -9's + 0.5 % at 0.9x.  4 .. 256, rounded down to a
                               multiple of 4. */
    void *stream;           /* hipStream_t to launch on (single-device ctx only); NULL = a stream owned by the ctx */
    /* ---- ABI 2 ---- */
    const int32_t *devices; /* n_devices HIP ordinals: the GPUs of the node this ctx shards over.  A single
                               entry of -1 means every visible device.  An ordinal may repeat
                               (two engines on one GPU: used by the tests on a 1-GPU box; RCCL needs distinct
                               devices, so the gather then falls back to per-device copies). */
    uint32_t n_devices;     /* 0 = the single `device` above */
    uint32_t host_threads;  /* planning (host entry points only; planner.h, snaphash_plan_streams below).  A lone SHA-512
                               stream advances at ~44 MB/s on the GPU whatever surrounds it and at ~1.4 GB/s on a host
                               core (the library's own vectorised SHA-512, hostsha.cpp); a launch costs ~0.15 ms.  Every
                               call is therefore planned: modelled GPU makespan = latency + max(longest stream / 44 MB/s,
                               bytes / PCIe link, fill work / fill threads), host makespan = LPT of the moved streams over
                               the host threads, and what all threads together ask of the cores; streams
                               move to host threads, longest first and concurrently with the GPU batch, while that
                               shortens the largest of the three -- the package's data.tar.gz (build.go:222), a 1 GiB member,
                               the few big files of a tree of many small ones, a share of a tree the link bounds -- and
                               a batch the host alone finishes sooner than any split (a lone file, a small tree dominated
                               by one member) runs on host threads whole: no call is slower than the reference's loop.
                                 0 (default) = the best of every host thread count up to what this process may keep busy
                                     (affinity mask capped by the cgroup CPU quota); the staging fill keeps its threads;
                                 N > 0 = exactly N;
                                 SNAPHASH_FLAG_GPU_ONLY = no planning, every byte through the HIP kernels.
                               snaphash_stats_ex says which bytes went where.  Not a fallback: init still fails
                               without a gfx950 device. */
    uint32_t flags;         /* SNAPHASH_FLAG_* */
    uint32_t reserved2;
} snaphash_config;

typedef struct snaphash_stats { /* of the most recent hashing call on the ctx */
    uint64_t bytes_hashed;  /* sum of file/buffer lengths */
    uint64_t blocks;        /* SHA-512 compression-function calls (incl. padding blocks) */
    uint64_t streams;       /* files/buffers hashed */
    uint32_t launches;      /* kernel launches issued */
    uint32_t kernel_used;   /* SNAPHASH_KERNEL_WIDE, _SPLIT or _PAIR (last launch) */
    double kernel_ms;       /* sum over launches, HIP events on the launch stream */
    double h2d_ms;          /* host->HBM copies (files/buffers entry points) */
    double wall_ms;         /* whole call, host clock */
} snaphash_stats;

typedef struct snaphash_stats_ex { /* of the most recent hashing call on the ctx */
    uint32_t struct_size;  /* in: sizeof(snaphash_stats_ex) */
    uint32_t n_devices;    /* engines the ctx shards over */
    uint32_t gather_kind;  /* 0 = none (one device), 1 = RCCL all-gather, 2 = per-device copies */
    uint32_t gather_checked; /* 1 = the RCCL result was compared with per-device copies and matched */
    double gather_ms;      /* digest gather, host clock */
    uint64_t gpu_bytes;    /* bytes hashed by HIP kernels */
    uint64_t host_bytes;   /* bytes hashed by host threads (hybrid scheduling; always 0 with SNAPHASH_FLAG_GPU_ONLY) */
    uint64_t host_streams; /* streams that were hashed on a host thread */
    uint64_t reserved3;    /* (ABI 2 declared a mid-stream hand-over counter here that was never implemented: whole
                              streams move or none) */
    double host_ms;        /* busiest host thread, host clock */
    /* ---- ABI 5 (filled when struct_size covers them; an ABI 4 caller's shorter struct is still accepted): what the
     * planner PREDICTED for the call set beside what the call then took.  A prediction off by more than a quarter says
     * that the model's constants do not describe this box (another PCIe generation, CPU or quota): snaphash_get_plan_model
     * shows them, and they are corrected from what the calls measure (planner.h PlanCalib). ---- */
    double planned_gpu_ms;  /* modelled makespan of the GPU part (0 = no plan: SNAPHASH_FLAG_GPU_ONLY, or no GPU part) */
    double planned_host_ms; /* modelled makespan of the host part (0 = none) */
    uint32_t planned_threads; /* host threads the plan asked for */
    uint32_t host_threads_run; /* host threads that ran (fewer when descriptors are short: snaphash.h, RLIMIT_NOFILE) */
    double gpu_ms;          /* actual: the GPU part from its first fill to its last digest, slowest engine, host clock */
    double hash_ms;         /* actual: planning + both parts + gather (the whole hashing step of the call; wall_ms of
                               snaphash_stats also holds the walk and the YAML of a tree call) */
    double plan_ms;         /* of that, the planner itself */
} snaphash_stats_ex;

/* ---- lifetime -------------------------------------------------------------- */
/* cfg == NULL: the calling thread's current device, defaults throughout -- unless the environment says otherwise
 * (the reference's build has neither config file nor flags for this): SNAPHASH_DEVICES = "all" or
 * "0,1,..." names the engines, SNAPHASH_HOST_THREADS = N sets the planner's host threads (0 = none: every
 * byte on the GPU), SNAPHASH_DEFLATE_DEPTH = N the producer's effort (deflate_depth).  A non-NULL cfg is taken as it
 * is; the environment is not consulted (but for SNAPHASH_KEEP_RLIMIT). */
int snaphash_init(const snaphash_config *cfg /* may be NULL */, snaphash_ctx **out);
void snaphash_destroy(snaphash_ctx *ctx);
int snaphash_abi_version(void);

/* ---- the primitive: helpers.Sha512sum, batched ----------------------------- */

/* Replaces n calls of helpers.Sha512sum(path) (helpers.go:188).  The library
 * opens and reads the files itself (pread into pinned staging -- two buffers, a
 * third for jobs of more than two -- H2D overlapped with the fill of the next,
 * chunked for files larger than a staging buffer).  digests: n*64 bytes.
 * status (may be NULL): per file 0 or the errno of the failed open/read. */
int snaphash_sha512_files(snaphash_ctx *ctx, const char *const *paths, size_t n,
                          uint8_t *digests, int32_t *status);

/* Same, for content already in host memory (what io.Copy would have streamed). */
int snaphash_sha512_buffers(snaphash_ctx *ctx, const void *const *bufs, const uint64_t *lens,
                            size_t n, uint8_t *digests);

/* Same, for content already resident in HBM: file i is the byte range
 * [d_base+offsets[i], +lens[i]).  offsets/lens are host arrays; every offset and
 * d_base must be 16-byte aligned, every length < 32 GiB.  d_digests is device memory, n*64 bytes.
 * Enqueues on the ctx stream and returns; snaphash_sync waits for completion.
 * This is the kernel-resident (roofline) entry point. */
int snaphash_sha512_device(snaphash_ctx *ctx, const void *d_base, const uint64_t *offsets,
                           const uint64_t *lens, size_t n, void *d_digests);
int snaphash_sync(snaphash_ctx *ctx);

/* One SHA-512 kernel alone over a job table of the caller's, on the caller's HBM: a test instrument, as
 * snaphash_xzenc_stages_device is one.  A job is one segment of one stream, what the library's own planners hand the
 * kernels (its internal Job, field for field). */
typedef struct snaphash_sha512_job {
    uint64_t data;       /* device address of the segment's first byte, 16-byte aligned */
    uint64_t nbytes;     /* bytes in this segment, < 32 GiB; a multiple of 128 unless the job is final */
    uint64_t total_prev; /* bytes of this stream hashed by earlier segments (the padding's length is total_prev + nbytes,
                          * a 64-bit byte count) */
    uint32_t idx;        /* the stream's row in d_state and d_digests */
    uint32_t flags;      /* SNAPHASH_JOB_FIRST | SNAPHASH_JOB_FINAL */
} snaphash_sha512_job;
#define SNAPHASH_JOB_FIRST 1u /* start from the initial hash value; otherwise from d_state[idx] */
#define SNAPHASH_JOB_FINAL 2u /* pad and write the digest to d_digests[idx]; otherwise the chaining value to d_state[idx] */
/* jobs[0..n) (host) go up in the caller's order -- NOT sorted longest first, as every other entry sorts them -- and
 * exactly one kernel runs over the whole table: kernel is SNAPHASH_KERNEL_WIDE, _SPLIT or _PAIR (_QUAD in a build that has
 * it); staged != 0 launches PAIR under its second name, sha512_pair_staged_kernel (other kernels have one name).
 * d_state: n_rows * 8 uint64 (a row's chaining value in host byte order), 8-byte aligned; d_digests: n_rows * 64 bytes,
 * 16-byte aligned.  A final job reads (unless first) its state row and writes its digest row; any other job writes its
 * state row; no other row and no byte outside the two arrays is written.  The kernels fetch 16 bytes at a time:
 * [data, data + round_up(nbytes, 16)) must be readable.  SNAPHASH_EINVAL: SNAPHASH_KERNEL_AUTO or an unknown kernel, an
 * address not 16-byte aligned, nbytes >= 2^35, a job that is not final whose nbytes is not a multiple of 128 or which is
 * first and empty (no planner builds one: there is nothing to carry yet), unknown flag bits, idx >= n_rows, two jobs with
 * one idx, a misaligned array, a streaming batch open on the ctx.  n == 0 does nothing.  Synchronous. */
int snaphash_sha512_jobs_device(snaphash_ctx *ctx, uint32_t kernel, int staged, const snaphash_sha512_job *jobs, size_t n,
                                size_t n_rows, void *d_state, void *d_digests);

/* ---- the pass: writeHashes / getHashes / Verify ----------------------------- */

/* writeHashes (build.go:216-270) minus the file write (north_star "getHashes"):
 * archive digest of data_tar + walk + per-file digests + yaml.v2-compatible text.
 * *yaml_out is malloc'd; release with snaphash_free. */
int snaphash_tree(snaphash_ctx *ctx, const char *build_dir, const char *data_tar,
                  char **yaml_out, size_t *yaml_len);

/* writeHashes itself: also MkdirAll(build_dir/DEBIAN, 0755) and writes
 * DEBIAN/hashes.yaml with mode 0644 (build.go:218-219, :269). */
int snaphash_write_hashes(snaphash_ctx *ctx, const char *build_dir, const char *data_tar);

typedef struct snaphash_mismatch {
    int32_t kind;     /* 1 missing on disk, 2 not in yaml, 3 size, 4 sha512, 5 mode, 6 archive-sha512 */
    int32_t reserved;
    char name[4096];  /* tree-relative name of the first offending record */
} snaphash_mismatch;

/* Inverse of writeHashes (absent upstream; hook point click.go:970): parse
 * yaml, re-walk inst_dir with the same rules, re-hash every regular file on the
 * GPU and compare name set, size, digest and mode.  data_tar may be NULL (the
 * archive digest is then not checked).  Returns 0, SNAPHASH_EMISMATCH (first
 * mismatch in *first, may be NULL) or another error. */
int snaphash_verify(snaphash_ctx *ctx, const char *inst_dir, const char *data_tar,
                    const char *yaml, size_t yaml_len, snaphash_mismatch *first);

/* snaphash_tree / snaphash_write_hashes with the archive digest supplied by the caller
 * (data_tar == NULL, archive_digest = the 64 raw bytes): the package's own data.tar.gz is ONE
 * stream, so the Go side hashes it with its existing crypto/sha512 code on a host core while the
 * GPU batch covers the tree.  With data_tar != NULL archive_digest is
 * ignored and the call equals snaphash_tree.  write != 0 also writes DEBIAN/hashes.yaml;
 * yaml_out may then be NULL. */
int snaphash_tree_ex(snaphash_ctx *ctx, const char *build_dir, const char *data_tar,
                     const uint8_t *archive_digest, int write, char **yaml_out, size_t *yaml_len);

void snaphash_free(void *p);

/* ---- streaming: hash while another pass reads ------------------ */

/* The reference reads every file twice in Build: tarCreate streams it into data.tar.gz
 * (clickdeb/deb.go:285-341), then writeHashes reads it again (snappy/build.go:228-259).  A batch
 * lets the producer feed each chunk it has just read, hash.Hash-style, so the bytes are read once:
 *   begin -> { append(stream, chunk) ... end(stream) } per file, streams may interleave -> finish.
 * append copies the bytes into pinned staging (the caller may reuse its buffer at once); full
 * staging buffers go to the GPU while the producer keeps reading; a stream's chaining value
 * stays in HBM between launches.  Streams are numbered 0 .. n_streams-1 by the caller.
 * finish pads and hashes what is left and writes n_streams digests (a stream that was never
 * appended to hashes as the empty file; a stream not ended is ended).  On a ctx with several devices the batch
 * runs on the first engine (a producer that feeds one chunk at a time is one PCIe link's worth of work at most).
 * Every byte of a batch goes through the kernels, where ONE stream advances at ~44 MB/s (the chain is serial): a batch
 * is for many streams of similar length.  A producer with long members among short ones hashes those itself, or hands
 * the whole pass to snaphash_tar_create, which sends a member whose chain would outlast the pass to a host thread
 * (reading it out of the staging buffer: still one read of every file). */
typedef struct snaphash_batch snaphash_batch;
int snaphash_batch_begin(snaphash_ctx *ctx, size_t n_streams, snaphash_batch **out);
int snaphash_batch_append(snaphash_batch *b, size_t stream, const void *data, size_t n);
int snaphash_batch_end(snaphash_batch *b, size_t stream);
int snaphash_batch_finish(snaphash_batch *b, uint8_t *digests /* n_streams * 64 */);
void snaphash_batch_abort(snaphash_batch *b);

/* ---- the data.tar.gz producer (fused with the hash pass: row f2) ---- */

typedef struct snaphash_targz_stats { /* of the most recent snaphash_tar_create / snaphash_gzip_buffer; after
                                       * snaphash_tar_create_xz / snaphash_xz_buffer: gz_bytes = bytes written, chunks = LZMA2
                                       * chunks of 65 536 bytes, stored_chunks = those written uncompressed, deflate_ms = the
                                       * chain, chunk, concatenation and CRC-64 kernels; after
                                       * snaphash_tar_create_bz2 / snaphash_bzip2_buffer: gz_bytes = bytes written, chunks =
                                       * bzip2 blocks, stored_chunks = 0 (bzip2 has no stored form), deflate_ms = all encoder
                                       * kernels (CRC, RLE1, BWT, MTF, coding, concatenation) */
    uint64_t tar_bytes;     /* uncompressed stream */
    uint64_t gz_bytes;      /* bytes written */
    uint64_t members;       /* tar members */
    uint64_t chunks;        /* 64 KiB deflate chunks (one DEFLATE block, one workgroup each) */
    uint64_t stored_chunks; /* of those, emitted as stored blocks (did not shrink) */
    double deflate_ms;      /* deflate + concatenation kernels, HIP events */
    double fill_ms;         /* assembling the tar stream in pinned memory (header records, parallel pread) */
    double wall_ms;
} snaphash_targz_stats;

/* tarCreate (clickdeb/deb.go:261-344): walks source_dir (filepath.Walk order, Lstat; regular files,
 * symlinks and directories only), skips every path that starts with exclude_prefix (NULL = none; Build
 * passes <source_dir>/DEBIAN, deb.go:361-363), names members "./<relative path>", owner root/root (ustar
 * headers; a name or link target they cannot hold travels in a PAX extended header, as archive/tar falls
 * back to; the size of a member of 8 GiB or more in the base-256 form), and writes the tar stream through a gzip member into tarname (must end in ".gz": the reference's ".xz"
 * branch is snaphash_tar_create_xz below).  The DEFLATE stream is produced on the GPU, block-parallel: it is
 * format-compatible with, not byte-identical to, compress/gzip level 9 (archive-sha512 is defined over
 * whatever bytes are produced, build.go:222).
 * yaml_out != NULL fuses writeHashes into the same pass (row f2: every file is read ONCE): the SHA-512
 * kernels hash each regular file out of the staged tar stream, the archive digest is taken over the
 * bytes written, and *yaml_out receives hashes.yaml (snaphash_free); exclude_prefix must then be
 * writeHashes' own rule.  A LONG member -- one whose SHA-512 chain would outlast its share of the pass on the GPU, where a
 * lone stream advances at ~44 MB/s -- is hashed by a host thread instead, out of the staging buffer the packer has read it
 * into (still one read; SNAPHASH_FLAG_GPU_ONLY keeps every byte on the kernels).
 * archive_digest (may be NULL): the 64 raw bytes of SHA-512(tarname).
 * tarname is created as os.Create does (deb.go:264) with one difference in timing: a file already there is
 * overwritten from offset 0 and cut to the new length when the last byte is written, not emptied first (emptying a
 * previous 250 MiB archive stalled the whole pipeline for 25-30 ms); it is unlinked when the pass fails.
 * On a ctx with several devices the producer runs on the first engine: the pass is bound by the one stream that
 * cannot be split -- the SHA-512 of the archive on a host core, 1.4 GB/s -- which a single PCIe link outruns 40x. */
int snaphash_tar_create(snaphash_ctx *ctx, const char *tarname, const char *source_dir, const char *exclude_prefix,
                        char **yaml_out, size_t *yaml_len, uint8_t *archive_digest);

/* The same with tarCreate's own third argument (clickdeb/deb.go:261: `fn tarExcludeFunc`, asked at deb.go:295-299):
 * keep(path, user) is called on the calling thread with the full path of every regular file, symlink and
 * directory of the walk, in walk order; zero leaves the entry out (a directory that is left out is still descended,
 * as in the reference, where fn returning false only skips that one entry).  NULL keeps everything.  From Go: an
 * //export'ed function as the callback, the closure's state behind `user`. */
typedef int (*snaphash_keep_fn)(const char *path, void *user);
int snaphash_tar_create_fn(snaphash_ctx *ctx, const char *tarname, const char *source_dir, snaphash_keep_fn keep, void *user,
                           char **yaml_out, size_t *yaml_len, uint8_t *archive_digest);

/* The compressor alone: one gzip member (RFC 1952) of a host buffer; *gz_out is malloc'd (snaphash_free). */
int snaphash_gzip_buffer(snaphash_ctx *ctx, const void *data, size_t n, void **gz_out, size_t *gz_len);

/* ---- the data.tar.xz producer (tarCreate's ".xz" branch, clickdeb/deb.go:272-273) ---- */

/* The .xz compressor alone, the twin of snaphash_gzip_buffer: one Stream of a host buffer (Check CRC-64, taken in HBM from
 * the staged bytes; the entry point below it takes the Check of the caller's choice), a Block per
 * block_size bytes -- a multiple of 64 KiB from 64 KiB to 4 MiB, 0 for the default of 1 MiB, anything else
 * SNAPHASH_EINVAL -- each Block header stating both sizes, as `xz -T` writes them; n == 0 gives a Stream without Blocks
 * (32 bytes).  Where the reference's `xz --compress --stdout` writes ONE Block, which any decoder reads on one thread,
 * every Block written here is one snaphash_unxz_buffer / snaphash_tar_unpack_xz decode side by side (also under
 * SNAPHASH_FLAG_GPU_ONLY: no Block is larger than the kernel takes).  Inside a Block the LZMA2 chunks (65 536 bytes
 * each) reset the coder state and keep the dictionary, so the GPU codes them side by side (lc=3 lp=0 pb=2; a hash-chain
 * match finder and a greedy parse: a little above `xz -0`'s size, well above `xz -6`'s).  The bytes are a function of
 * (data, block_size) alone.  *xz_out is malloc'd (snaphash_free).  The engine's staging size must hold a Block. */
int snaphash_xz_buffer(snaphash_ctx *ctx, const void *data, size_t n, uint64_t block_size, void **xz_out, size_t *xz_len);
/* The same with the Check of the caller's choice, each taken in HBM by its kernel: 0 none, 1 CRC-32, 4 CRC-64 (then byte
 * for byte the output of the call above), 10 SHA-256 (what `xz -C sha256` writes: the one cryptographic Check of the
 * format); anything else SNAPHASH_EINVAL.  The Stream flags of header and footer carry the id; the Index follows its size. */
int snaphash_xz_buffer_check(snaphash_ctx *ctx, const void *data, size_t n, uint64_t block_size, uint32_t check,
                             void **xz_out, size_t *xz_len);
/* snaphash_tar_create for a data.tar.xz: the same walk, tar layout, single read, fused hashes.yaml, late truncation and
 * unlink-on-failure; tarname must end in ".xz" (anything else: SNAPHASH_EINVAL, "unknown compression extension").
 * Blocks of 1 MiB; a Block never spans two staging slots.  snaphash_get_targz_stats reports the pass. */
int snaphash_tar_create_xz(snaphash_ctx *ctx, const char *tarname, const char *source_dir, const char *exclude_prefix,
                           char **yaml_out, size_t *yaml_len, uint8_t *archive_digest);

/* The two producers above with the caller's Block size and Check, and with the producer's self-check. */
enum { SNAPHASH_XZ_SELF_CHECK = 1 }; /* every LZMA2 chunk is walked against the staged bytes it was made from, in HBM, before
                                      * it leaves the GPU: a chunk that would not decode back fails the call (SNAPHASH_EDEVICE;
                                      * snaphash_last_error names the Block, the chunk, the status -- snaphash_lzma2_verdict's --
                                      * and the offset in the uncompressed stream; a file being written is unlinked).  The bytes
                                      * written are the same with and without it.  Not covered: Block headers, padding,
                                      * Check fields, Index and footer (written on the host), the copy back and the write;
                                      * decoding the file covers those. */
typedef struct snaphash_xz_options {
    uint32_t struct_size; /* sizeof(snaphash_xz_options) */
    uint32_t flags;       /* SNAPHASH_XZ_*; an unknown bit is SNAPHASH_EINVAL */
    uint64_t block_size;  /* as in snaphash_xz_buffer: 0 = 1 MiB */
    uint32_t check;       /* as in snaphash_xz_buffer_check: 0 none, 1 CRC-32, 4 CRC-64, 10 SHA-256 */
    uint32_t filter;      /* a BCJ filter in front of LZMA2, by the format's id: 0 none, 4 x86, 7 ARM, 8 ARM-Thumb; anything
                           * else is SNAPHASH_EINVAL.  (The field was `reserved`, 0, at this offset and size.)  See below. */
    uint32_t level;       /* 0: the greedy parse, one candidate a position (what every entry without a level writes, byte for
                           * byte); 1: several candidates a position and a price-based shortest-path parse:
                           * smaller files for more kernel time.  Anything else is SNAPHASH_EINVAL.  Read when struct_size >= 32;
                           * a struct_size of 24, the struct before this field, means level 0. */
    uint32_t reserved2;   /* 0; anything else is SNAPHASH_EINVAL */
    uint32_t chain_len;   /* 0 .. 3: the filters in front of LZMA2 when they are more than `filter` can say.
                           * Read, with chain, when struct_size >= 48; sizes 24 and 32 .. 47 mean what they meant. */
    uint32_t chain[3];    /* chain[k] = id | param << 8, the Block header's first filter first: id 3 Delta with param its
                           * distance 1 .. 256, ids 4 x86, 5 PowerPC, 6 IA64, 7 ARM, 8 ARM-Thumb, 9 SPARC with param 0 (their
                           * start_offset is 0).  Any order, repeats allowed.  SNAPHASH_EINVAL, touching nothing: chain_len
                           * above 3, an id outside 3 .. 9, a distance of 0 or above 256, a param on a BCJ id, `filter` and
                           * chain_len both nonzero (`filter` itself keeps to 0, 4, 7, 8).  chain = {4} writes byte for byte
                           * what filter = 4 writes.  Delta is named with its one property byte, the others with none; the
                           * Checks, the members' SHA-512 and hashes.yaml stay over the unfiltered bytes; the self-check walks
                           * the chunks against the filtered bytes, undoes the whole chain in place and compares with the
                           * staged bytes.  snaphash_unxz_buffer_ex with SNAPHASH_UNXZ_CHAINS reads the file back. */
} snaphash_xz_options;
typedef struct snaphash_xz_selfcheck_stats {
    uint32_t struct_size; /* set by the caller */
    uint32_t reserved;
    uint64_t chunks;      /* LZMA2 chunks walked (all accepted, or the call failed); 0 without SNAPHASH_XZ_SELF_CHECK */
    double ms;            /* the check kernel's own time, HIP events */
} snaphash_xz_selfcheck_stats;
/* opt == NULL, or a struct that is all zero (struct_size included): byte for byte what snaphash_xz_buffer /
 * snaphash_tar_create_xz write (1 MiB Blocks, CRC-64, no self-check, level 0).  Otherwise struct_size says the struct's size
 * -- 24 (the struct without level and reserved2) or at least 32 -- and every field means what it says.  SNAPHASH_EINVAL: any
 * other struct_size, an unknown flag, a refused Block size, an unknown Check id, a level above 1, a nonzero reserved2.  A
 * refused call touches nothing.  At any level the bytes are a function of (data, the options) alone, and the file differs
 * from level 0's only in the LZMA2 chunks' contents: the self-check, the filters and the install side take it as it is. */
int snaphash_xz_buffer_ex(snaphash_ctx *ctx, const void *data, size_t n, const snaphash_xz_options *opt, void **xz_out,
                          size_t *xz_len);
int snaphash_tar_create_xz_ex(snaphash_ctx *ctx, const char *tarname, const char *source_dir, const char *exclude_prefix,
                              const snaphash_xz_options *opt, char **yaml_out, size_t *yaml_len, uint8_t *archive_digest);
/* of the most recent call among the two _ex calls above and snaphash_snap_build with a data.tar.xz (the data member's) */
int snaphash_get_xz_selfcheck_stats(const snaphash_ctx *ctx, snaphash_xz_selfcheck_stats *out);
/* snaphash_xz_options.filter.  A snap's data member is mostly machine code; a BCJ (branch-call-jump)
 * filter rewrites the relative targets of calls and jumps as absolute ones, so that calls of one function become equal
 * bytes for LZMA2.  With a filter every Block's chain is that filter (no properties: start_offset 0) followed by LZMA2,
 * the chain `xz --x86 --lzma2` writes; liblzma and snaphash_unxz_buffer_ex with SNAPHASH_UNXZ_BCJ read it.  The slot's staged
 * bytes are copied once more in HBM, the copy is filtered in place by the BCJ kernels (a Block a range, positions from the
 * Block's first byte, so Blocks stay independent), and the LZMA2 kernels read the copy; the Blocks' Checks, the members'
 * SHA-512 and hashes.yaml are taken from the unfiltered bytes, as the format asks.  filter == 0 writes byte for byte what
 * the struct wrote before the field had a name.  SNAPHASH_XZ_SELF_CHECK with a filter walks the chunks against the filtered
 * bytes, then undoes the filter in place and compares the result with the staged bytes in HBM: a difference is
 * SNAPHASH_EDEVICE, snaphash_last_error naming the Block and the offset. */

typedef struct snaphash_lzma2_verdict {
    uint32_t status; /* 0 accepted; 1 a literal or stored byte differs; 2 a match's or short rep's copy differs; 3 a distance
                        beyond the bytes in front of the position in its Block (or block_size); 4 not the producer's LZMA2
                        (control byte, properties, dictionary reset inside a Block, first range coder byte not zero, end
                        marker, input overrun); 5 a match longer than what is left of the chunk; 6 the header's uncompressed
                        size is not the chunk's; 7 sizes or the coder's end do not meet the stretch's end (a missing, non-zero
                        or misplaced end byte too); 8 the table entry lies outside the compressed bytes, or z_end < z_beg */
    uint32_t offset; /* within the chunk: the first byte that differs, else how far the walk had come */
} snaphash_lzma2_verdict;
/* The self-check kernel alone, on tables the caller wrote (tests): d_in[0..n_in) is the staged stream in HBM, cut into Blocks
 * of block_size bytes (as in snaphash_xz_buffer) and nchunks == ceil(n_in / 65536) chunks; d_z[0..n_z) holds the compressed
 * bytes, chunk c's stretch being [z_beg[c], z_end[c]) (host arrays).  A chunk is accepted when its stretch is ONE LZMA2 chunk
 * of the producer's form -- a Block's first 0xE0|.. with properties 0x5D or 0x01, a later one 0xC0|.. with 0x5D or 0x02 --
 * whose uncompressed size is the chunk's, that ends exactly at the stretch's end (behind the 0x00 end byte for a Block's last
 * chunk, which no other stretch may include), whose coder consumes every compressed byte and ends with code == 0, and whose
 * every byte and every match, taken from the staged stream, equals the staged bytes.  One launch takes launch_chunks chunks
 * (0: 2048, the most allowed).  verdicts: nchunks entries (host).  Nothing is written to the caller's HBM.
 * SNAPHASH_EINVAL: a null pointer, n_in == 0, a refused block size, nchunks other than ceil(n_in / 65536), launch_chunks >
 * 2048.  Synchronous. */
int snaphash_lzma2_check_device(snaphash_ctx *ctx, const void *d_in, size_t n_in, uint64_t block_size, const void *d_z, size_t n_z,
                                const uint64_t *z_beg, const uint64_t *z_end, size_t nchunks, uint32_t launch_chunks,
                                snaphash_lzma2_verdict *verdicts);
void snaphash_get_targz_stats(const snaphash_ctx *ctx, snaphash_targz_stats *out);
/* The compressor's Huffman code construction alone, by the routines the chunk kernel runs (a wave per table): for callers
 * who want to check them, as the tests do.  d_freq: n_tables tables of n_syms uint32 symbol counts each, resident in HBM.
 * Per table, to the caller's HBM: d_lens, n_syms bytes -- the code lengths (0 for a count of 0, 1 for a lone used symbol,
 * otherwise a complete prefix code of at most max_bits); d_codes, n_syms uint32 -- the canonical code of every symbol,
 * bit-reversed for the LSB-first stream, << 8 | its length (0 for no code); d_rounds, one uint32 -- the trees built:
 * 1 when the first fitted max_bits, one more for every halving of the counts (a count is never halved to 0, and counts
 * above 65535 weigh 65535).  No byte outside the three arrays is written.  SNAPHASH_EINVAL unless 1 <= n_syms <= 320,
 * 1 <= max_bits <= 15 and n_syms <= 2^max_bits.  Synchronous. */
int snaphash_deflate_codes_device(snaphash_ctx *ctx, const void *d_freq, size_t n_tables, uint32_t n_syms, uint32_t max_bits,
                                  void *d_lens, void *d_codes, void *d_rounds);

/* The .xz encoder's three kernels alone, on the caller's HBM: what snaphash_xz_buffer / snaphash_tar_create_xz run for one
 * staged piece d_in[0..n) (the same steps in the same order, in a routine of this entry's own), cut
 * into Blocks of block_size bytes (as in snaphash_xz_buffer; the last Block may be short) -- lzma_chains_kernel,
 * lzma2_chunks_kernel in launches of launch_chunks chunks (0: the producer's 2048, the most allowed), the results back to
 * the host, every Block's layout, the chunks' places up to the device, lzma2_concat_kernel.  With nch = ceil(n / 65536):
 *   d_prev, d_cand   n uint32 each: the hash chains (Block-relative, 0xffffffff for none) and the candidates
 *                    (length << 22 | distance - 1, 0 for none)
 *   d_slots          nch * 65600 bytes: every chunk's coder output from its slot's first byte (what does not fit is
 *                    counted, not stored)
 *   d_res            nch uint32: a chunk's compressed size, or 0x80000000 for one written uncompressed
 *   d_dst            nch uint64: where a chunk's header goes in d_out
 *   d_out            out_cap >= n + nch * 64 + 64 bytes: the Blocks one after another, chunk headers, bodies and each
 *                    Block's end byte in place.  Block headers, Block Padding and Checks are NOT written: those bytes
 *                    stay what the caller put there.
 * block_total (host, may be NULL): a uint64 a Block, its bytes in d_out (header, data, padding, Check).  No byte outside
 * the six arrays is written.  SNAPHASH_EINVAL: a refused block size, launch_chunks > 2048, out_cap too small, a null
 * pointer with n > 0.  n == 0 does nothing.  Synchronous. */
int snaphash_xzenc_stages_device(snaphash_ctx *ctx, const void *d_in, size_t n, uint64_t block_size, uint32_t launch_chunks,
                                 void *d_prev, void *d_cand, void *d_slots, void *d_res, void *d_dst, void *d_out, size_t out_cap,
                                 uint64_t *block_total);
/* The same at a level (snaphash_xz_options.level; above 1: SNAPHASH_EINVAL): level 0 is the entry above, byte for byte.  At
 * level 1 the chunks are coded by lzma2_chunks_priced_kernel and d_cand holds 4 uint32 per byte of the piece, 4 n in all: a
 * position's candidates nearest first, lengths strictly rising, 0 behind the last; launch_chunks 0 is then the producer's 768. */
int snaphash_xzenc_stages_device_ex(snaphash_ctx *ctx, const void *d_in, size_t n, uint64_t block_size, uint32_t launch_chunks,
                                    void *d_prev, void *d_cand, void *d_slots, void *d_res, void *d_dst, void *d_out, size_t out_cap,
                                    uint64_t *block_total, uint32_t level);

/* ---- the data.tar.bz2 producer (the one format ClickDeb.Unpack reads, deb.go:185, and tarCreate refuses to write) ---- */

/* One bzip2 stream of a host buffer; level 1..9 (0 = 9), anything else SNAPHASH_EINVAL; n == 0 gives the 14-byte stream
 * without blocks; *bz_out is malloc'd (snaphash_free).  The input is cut into blocks by INPUT size -- 719 872 bytes at
 * level 9, 79 872 at level 1: floor((100 000 level - 19) * 4/5 / 512) * 512, what RLE1 can never expand past libbz2's own
 * block size -- so every block is coded side by side on the GPU: RLE1, the Burrows-Wheeler transform by prefix doubling
 * with radix passes, move-to-front, libbz2's Huffman scheme (2-6 tables, four refinement rounds, codes of up to 17 bits).
 * Any bzip2 decoder reads the file, block-parallel ones side by side.  The bytes are a function of (data, level) alone.
 * The engine's staging size must hold a block's input. */
int snaphash_bzip2_buffer(snaphash_ctx *ctx, const void *data, size_t n, uint32_t level, void **bz_out, size_t *bz_len);

/* snaphash_tar_create for a data.tar.bz2 (level 9): same walk, tar layout, single read, fused hashes.yaml, host-thread
 * member digests, late truncation, unlink on failure; tarname must end in ".bz2", else SNAPHASH_EINVAL with
 * "unknown compression extension".  A block never spans two staging slots.  snaphash_get_targz_stats reports the pass. */
int snaphash_tar_create_bz2(snaphash_ctx *ctx, const char *tarname, const char *source_dir, const char *exclude_prefix,
                            char **yaml_out, size_t *yaml_len, uint8_t *archive_digest);

/* Test instrument, like snaphash_deflate_codes_device: the BWT stage alone over n_blocks ranges of a caller's HBM buffer
 * (offsets / lens: host arrays; each range 1..900 000 bytes, taken as it is: no RLE1), by the kernel the encoder runs.
 * d_last receives each range's last column of its sorted cyclic rotations at the range's own offset, d_orig_ptr one uint32
 * per range: the number of rotations that sort before rotation 0 (equal rotations by start index).  No byte outside those
 * is written, d_in is only read.  Ranges that overlap give undefined last columns.  Synchronous. */
int snaphash_bwt_device(snaphash_ctx *ctx, const void *d_in, const uint64_t *offsets, const uint64_t *lens, size_t n_blocks,
                        void *d_last, void *d_orig_ptr);

/* Test instrument, like snaphash_xzenc_stages_device: the .bz2 producer's sequence for one staged slot, step for step --
 * the job table, the blocks' CRCs, RLE1 / BWT / MTF / coding in one launch each, the host's placement of the blocks with its
 * check of what the stages reported, the concat kernel -- over n_blocks ranges of d_in taken as they are (offsets / lens:
 * host arrays, as snaphash_bwt_device takes them; each range 1 byte to the level's piece, (100 000 x level - 19) x 4 / 5
 * rounded down to 512), with every per-block array but the sort's scratch in the caller's HBM, block k at k strides:
 *   d_rle, d_last   cap + 64 bytes          RLE1's output, the BWT's last column
 *   d_syms          cap + 64 uint16         the MTF / RUNA / RUNB symbols, the end-of-block symbol last
 *   d_maps          516 bytes               used[256], seq[256], nused (uint32)
 *   d_sel           18 048 bytes            a selector a group of 50 symbols
 *   d_slots         W(cap) uint32           the block's bits from bit 0, zero behind them; W(cap) = (159 521 + 17 x (cap + 1)
 *                                           + 31) / 32 + 2: the header's worst case and 17 bits a symbol
 *   d_res           6 uint32                rle_n, orig_ptr, nmtf, bits, over, 0
 *   d_dst           uint64                  the bit of d_out the block starts at
 *   d_out           out_words uint32 in all the blocks shifted together, zero behind the last bit
 * level: 1 to 9.  cap: the longest RLE1 output a block may have, a multiple of 64 up to 899 840; 0: the producer's, the
 * level's piece x 5 / 4 rounded up to 64.  carry / carry_bits: the carry_bits (< 8) bits that precede block 0 in byte 0 of
 * d_out, left-aligned in a byte, the rest of it zero.  At most 1024 blocks, and n_blocks x cap <= 32 x 899 840.
 * rle_n != NULL is the from_last mode: RLE1 and the BWT are not run; the caller has put block k's last column, rle_n[k]
 * (1 to cap) bytes, into d_last, and orig_ptr[k] (< rle_n[k]) and crc[k] are what the header is to say; d_in, offsets,
 * lens and d_rle are not looked at.  Otherwise rle_n, orig_ptr and crc are NULL.
 * Returns SNAPHASH_OK and *total_bits, the bit behind the last block (carry_bits included).  SNAPHASH_EINVAL, before anything
 * is launched: a range or a column outside its limits, orig_ptr >= rle_n, a bad level, cap or carry, a NULL array; and,
 * once the blocks' lengths are known and before d_dst and d_out are written, out_words below (total bits + 31) / 32.  A
 * block whose RLE1 output exceeds cap stores what fits into its cap + 64 bytes and reports rle_n 0 and over 1; then, and
 * for any other result the producer refuses, the call fails as the producer does: SNAPHASH_EDEVICE, "bzip2: a block's stages
 * reported an impossible result", d_dst and d_out untouched, the other arrays as the kernels left them.  No byte outside
 * the arrays as sized above is written, d_in is only read.  Ranges may overlap.  Synchronous. */
int snaphash_bzenc_stages_device(snaphash_ctx *ctx, const void *d_in, const uint64_t *offsets, const uint64_t *lens, size_t n_blocks,
                                 uint32_t level, uint32_t cap, uint32_t carry, uint32_t carry_bits, const uint32_t *rle_n,
                                 const uint32_t *orig_ptr, const uint32_t *crc, void *d_rle, void *d_last, void *d_syms, void *d_maps,
                                 void *d_sel, void *d_slots, void *d_res, void *d_dst, void *d_out, size_t out_words,
                                 uint64_t *total_bits);

/* The two producers above with the caller's level, and with the producer's self-check. */
enum { SNAPHASH_BZ2_SELF_CHECK = 1 }; /* every block is decoded again in HBM -- symbols, inverse BWT, RLE1 -- and compared with
                                       * the staged piece it was made from before it leaves the GPU: a block that would not
                                       * decode back fails the call (SNAPHASH_EDEVICE; snaphash_last_error names the member,
                                       * the block, the status -- snaphash_bz2_verdict's -- and the offset in the uncompressed
                                       * stream; a file being written is unlinked).  The bytes written are the same with and
                                       * without it.  Not covered: "BZh" + level, the end-of-stream magic and the combined CRC
                                       * (written on the host), the copy back and the write; decoding the file covers those.
                                       * Adds the install side's decode scratch: 4.5 MB a block of a staging slot, 256 blocks
                                       * at most. */
typedef struct snaphash_bz2_options {
    uint32_t struct_size; /* sizeof(snaphash_bz2_options) */
    uint32_t flags;       /* SNAPHASH_BZ2_*; an unknown bit is SNAPHASH_EINVAL */
    uint32_t level;       /* as in snaphash_bzip2_buffer: 1..9, 0 = 9 */
} snaphash_bz2_options;
typedef struct snaphash_bz2_selfcheck_stats {
    uint32_t struct_size; /* set by the caller */
    uint32_t reserved;
    uint64_t blocks;      /* blocks decoded again (all accepted, or the call failed); 0 without SNAPHASH_BZ2_SELF_CHECK */
    double ms;            /* the check's kernels' own time, HIP events */
} snaphash_bz2_selfcheck_stats;
/* opt == NULL, or a struct that is all zero (struct_size included): byte for byte what snaphash_bzip2_buffer(level 9) /
 * snaphash_tar_create_bz2 write.  Otherwise struct_size says the struct's size and every field means what it says.
 * SNAPHASH_EINVAL, and the ctx stays usable: an unknown flag, another struct_size, a level above 9.
 * snaphash_tar_create_bz2_ex is the tar entry that gives .bz2 a level. */
int snaphash_bzip2_buffer_ex(snaphash_ctx *ctx, const void *data, size_t n, const snaphash_bz2_options *opt, void **bz_out,
                             size_t *bz_len);
int snaphash_tar_create_bz2_ex(snaphash_ctx *ctx, const char *tarname, const char *source_dir, const char *exclude_prefix,
                               const snaphash_bz2_options *opt, char **yaml_out, size_t *yaml_len, uint8_t *archive_digest);
/* of the most recent call among the two _ex calls above and snaphash_snap_build with a data.tar.bz2 (the data member's) */
int snaphash_get_bz2_selfcheck_stats(const snaphash_ctx *ctx, snaphash_bz2_selfcheck_stats *out);

typedef struct snaphash_bz2_verdict {
    uint32_t status; /* in order of precedence: 0 accepted; 8 the table entry lies outside the compressed bytes, or z_end < z_beg,
                        or the piece lies outside the staged buffer (nothing was read); 3 no valid block at z_beg (magic,
                        randomised bit, maps, selectors, tables, truncated, empty); 4 more symbols than 100 000 x level; 7 origPtr
                        >= n, or the inverse BWT's walk breaks; 5 the block does not end at z_end; 6 the stored block CRC is not
                        the piece's; 1 a byte differs; 2 all of min(decoded, in_len) bytes agree and the lengths differ */
    uint32_t offset; /* 0: in_len; 8, 6: 0; 3: the block reader's own status (2 truncated, 4 bad); 4: the cap; 7: origPtr; 5: the
                        low 32 bits of the block's end bit - z_beg; 1: the first differing byte within the piece; 2: the minimum */
} snaphash_bz2_verdict;
/* The self-check's four steps alone, on tables the caller wrote (tests): d_z[0..n_z) holds compressed bytes in HBM, block k's
 * bits being [z_beg[k], z_end[k]) (bit offsets, MSB first; host arrays); d_in[0..n_in) is the staged stream in HBM, block k's
 * piece being d_in[in_off[k] .. in_off[k] + in_len[k]) and crc[k] the bzip2 CRC the caller holds for it; level: the stream's,
 * 1..9.  Any valid bzip2 block is taken, not only this library's.  verdicts: n_blocks entries (host).  Nothing is written to
 * the caller's HBM; nothing outside d_z[0..n_z) and the blocks' pieces is read.  SNAPHASH_EINVAL: a null pointer, a level
 * outside 1..9.  Synchronous. */
int snaphash_bz2_check_device(snaphash_ctx *ctx, const void *d_z, size_t n_z, const uint64_t *z_beg, const uint64_t *z_end,
                              const void *d_in, size_t n_in, const uint64_t *in_off, const uint64_t *in_len, const uint32_t *crc,
                              uint32_t level, size_t n_blocks, snaphash_bz2_verdict *verdicts);

/* ---- the install side: data.tar.gz unpacked and verified in one read ---------------------- */

typedef struct snaphash_unpack_stats { /* of the most recent snaphash_gunzip_buffer / snaphash_tar_unpack, or of the
                                        * bzip2 calls (snaphash_bunzip2_buffer / snaphash_tar_unpack_bz2), where the fields
                                        * mean what the comment after each one's semicolon says, or of the xz calls
                                        * (snaphash_unxz_buffer / snaphash_tar_unpack_xz: segments = Blocks, gpu_segments =
                                        * Blocks the kernel decoded, host_bytes = output of the Blocks decoded on the
                                        * host, inflate_ms = the decode and Check kernels) */
    uint32_t struct_size;   /* in: sizeof(snaphash_unpack_stats) */
    uint32_t reserved;
    uint64_t gz_bytes;      /* compressed input (bzip2: the same) */
    uint64_t tar_bytes;     /* decoded output */
    uint64_t members;       /* tar members (0 for snaphash_gunzip_buffer) */
    uint64_t segments;      /* stretches the stream was decoded in: linked GPU segments + host stretches (bzip2: blocks) */
    uint64_t gpu_segments;  /* of those, decoded by the inflate kernel (bzip2: blocks the bzip2 kernels decoded) */
    uint64_t host_bytes;    /* output bytes the host decoder produced (stretches without flush points, gaps; bzip2: the
                               blocks decoded on host threads) */
    double inflate_ms;      /* inflate kernels (scan, decode, fill, concat), HIP events (bzip2: the decode kernels --
                               scan, symbols, inverse BWT, RLE1) */
    double wall_ms;
} snaphash_unpack_stats;

/* The inverse of snaphash_gzip_buffer: every member of gz[0..n) (RFC 1952; concatenated members are read one after
 * another, as Go's gzip.Reader does), each member's CRC-32 and ISIZE checked.  *out is malloc'd (snaphash_free).
 * The DEFLATE stream is cut at its flush points (the empty stored block of Z_SYNC_FLUSH, which the producer writes after
 * every 64 KiB chunk, and stored blocks) and the segments are decoded side by side -- on host threads in the default
 * configuration (measured faster), by the GPU inflate kernel under SNAPHASH_FLAG_GPU_ONLY; a stretch without flush points
 * (zlib's or Go's plain output) and any segment the kernel gives up on are decoded by the host decoder.
 * SNAPHASH_EFORMAT: not a gzip / DEFLATE stream, or a CRC-32 / ISIZE mismatch. */
int snaphash_gunzip_buffer(snaphash_ctx *ctx, const void *gz, size_t n, void **out, size_t *out_len);
/* SNAPHASH_FLAG_SPLIT_BLOCKS (opt-in; the same bytes out, or the same error): a member that starts with at least 1 MiB
 * of the stream left is cut at its DEFLATE block boundaries too, not only at flush points (a member's length is not
 * known before it is decoded: its first piece is 1 MiB, later ones the engine's piece size).  A GPU kernel
 * tests every bit offset for a dynamic-Huffman block header that the decoder accepts; those starts, the stored-block
 * ends and the piece's start are decoded side by side as above (host threads / the inflate kernel, from any bit), each
 * segment stopping at the first block end after 16 Ki output symbols where a dynamic block follows or a stored block
 * ended; the chain is linked from the member's start, a false start drops out.  Where the chain breaks (a block longer
 * than a slot, a run of fixed blocks at a piece's start) the host decoder takes the stretch to the next block the scan
 * can find, and the chain resumes there.  The unpack statistics keep their meaning: host_bytes counts only that host
 * decoder's output; snaphash_get_block_scan_stats tells what the scan and the link did.  A member with less than 1 MiB
 * of the stream left, and every stream without the flag, take the route above. */

/* ClickDeb.Unpack (clickdeb/deb.go:188-203) of data.tar.gz into target_dir: helpers.UnpackTar (helpers/helpers.go:74-147)
 * with clickVerifyContentFn (deb.go:96-103) -- every name through filepath.Clean, any that still contains ".." refused
 * (SNAPHASH_ECONTENT); MkdirAll(dir, 0777) for every member; a directory Mkdir'ed with its mode (an error ignored); a
 * symlink created; a regular file opened O_WRONLY|O_TRUNC|O_CREAT with its mode (the umask applies); PAX extended headers
 * and GNU long names read as archive/tar reads them; any other member type refused (SNAPHASH_ECONTENT); the first error
 * stops the call.  yaml != NULL also does the install-time Verify of hashes.yaml (click.go:955-970) without reading a
 * file back: every regular member is hashed from the decoded stream in HBM (long ones on host threads, as the producer
 * plans them; SNAPHASH_FLAG_GPU_ONLY keeps them on the kernels), the archive digest is taken over the compressed bytes,
 * and the result is 0 or SNAPHASH_EMISMATCH with the kind and name snaphash_verify reports on the unpacked tree.
 * archive_digest (may be NULL): the 64 raw bytes of SHA-512(data_tar_gz). */
int snaphash_tar_unpack(snaphash_ctx *ctx, const char *data_tar_gz, const char *target_dir, const char *yaml, size_t yaml_len,
                        snaphash_mismatch *first, uint8_t *archive_digest);
/* out->struct_size in; SNAPHASH_EINVAL if it is smaller than the ABI 5 struct. */
int snaphash_get_unpack_stats(const snaphash_ctx *ctx, snaphash_unpack_stats *out);

typedef struct snaphash_block_scan_stats { /* SNAPHASH_FLAG_SPLIT_BLOCKS: of the most recent snaphash_gunzip_buffer /
                                            * snaphash_tar_unpack (all zero without the flag, or when every member
                                            * started with less than 1 MiB of the stream left) */
    uint32_t struct_size;    /* in: sizeof(snaphash_block_scan_stats) */
    uint32_t reserved;
    uint64_t bits_scanned;   /* bit offsets the block scan tested (a piece's tail the chain did not reach is scanned again) */
    uint64_t candidates;     /* offsets the scan accepted: dynamic-Huffman block headers the decoder accepts */
    uint64_t linked;         /* segments linked from a block candidate */
    uint64_t unreached;      /* candidates the link never reached: false ones, or inside a segment (candidates - linked) */
    uint64_t host_blocks;    /* stretches the host decoder took because the chain broke */
    double scan_ms;          /* block scan kernel time, HIP events */
} snaphash_block_scan_stats;
/* out->struct_size in; SNAPHASH_EINVAL if it is smaller than this struct. */
int snaphash_get_block_scan_stats(const snaphash_ctx *ctx, snaphash_block_scan_stats *out);

/* ---- the install side for data.tar.bz2 (skipToArMember's ".bz2" branch, clickdeb/deb.go:408-441) ----------------- */

/* Every stream of bz[0..n) ("BZh" + level 1-9; concatenated streams read one after another, pbzip2's output among
 * them), every block CRC and each stream's combined CRC checked.  *out is malloc'd (snaphash_free).  bzip2 blocks need
 * nothing from each other: they are decoded side by side -- on host threads in the default configuration (measured
 * faster than one core of libbz2), by the GPU bzip2 kernels under SNAPHASH_FLAG_GPU_ONLY (block scan,
 * Huffman + MTF decode, inverse BWT, RLE1 undo), any block the kernels give up on by the host decoder.
 * SNAPHASH_EFORMAT, as Go's compress/bzip2 refuses them: not a bzip2 stream, n == 0, a block or combined CRC mismatch,
 * the randomised bit set, origPtr out of range, a block longer than its level allows, trailing bytes that are not
 * another stream. */
int snaphash_bunzip2_buffer(snaphash_ctx *ctx, const void *bz, size_t n, void **out, size_t *out_len);
/* snaphash_tar_unpack for a data.tar.bz2: the same UnpackTar rules, errors and in-pass Verify, from the bzip2-decoded
 * stream; archive_digest (may be NULL): the 64 raw bytes of SHA-512(data_tar_bz2). */
int snaphash_tar_unpack_bz2(snaphash_ctx *ctx, const char *data_tar_bz2, const char *target_dir, const char *yaml,
                            size_t yaml_len, snaphash_mismatch *first, uint8_t *archive_digest);

/* ---- the install side for data.tar.xz (skipToArMember's ".xz" branch, clickdeb/deb.go:408-441) ------------------- */

/* Every Stream of xz[0..n) (the .xz file format: Stream Padding and concatenated Streams read as the xz tool reads them;
 * a Stream without Blocks decodes to nothing), every header, Index and footer CRC-32 and every Block's Check verified
 * (none, CRC-32, CRC-64, SHA-256).  *out is malloc'd (snaphash_free).  The Index gives every Block's place in the file and
 * in the result before a byte is decoded, and a Block needs nothing from another: they are decoded side by side, each
 * straight to its final offset -- a Block a host thread in the default configuration, a Block a workgroup of
 * lzma2_blocks_kernel under SNAPHASH_FLAG_GPU_ONLY, with the CRC-32, CRC-64 and SHA-256 Checks of those Blocks taken in HBM
 * (a range a Block: the CRC kernels, sha256_ranges_kernel).  Inside one Block LZMA is a serial chain: a file of one Block
 * (what `xz` writes without -T or --block-size) decodes on one thread.  A Block of more than 4 MiB of output, and any
 * Block the kernel gives up on, is decoded and checked by a host thread in either configuration.
 * In the unpack statistics segments = Blocks, gpu_segments = Blocks the kernel decoded, host_bytes = output of the
 * Blocks decoded on the host, inflate_ms = the decode and Check kernels.
 * SNAPHASH_EFORMAT: whatever liblzma refuses -- a wrong magic or CRC, an Index that disagrees with its Blocks, malformed
 * LZMA2, a Check mismatch, bytes behind the last Stream that are neither padding nor a Stream, n == 0.
 * SNAPHASH_EINVAL: a well-formed file this decoder does not take -- a filter chain other than one LZMA2 ("xz:
 * unsupported filter 0xNN": the BCJ filters, delta; snaphash_unxz_buffer_ex below takes three of the former) or a Check id other than 0, 1, 4, 10; the caller decodes it itself. */
int snaphash_unxz_buffer(snaphash_ctx *ctx, const void *xz, size_t n, void **out, size_t *out_len);
/* snaphash_tar_unpack for a data.tar.xz: the same UnpackTar rules, errors and in-pass Verify, from the xz-decoded
 * stream; archive_digest (may be NULL): the 64 raw bytes of SHA-512(data_tar_xz). */
int snaphash_tar_unpack_xz(snaphash_ctx *ctx, const char *data_tar_xz, const char *target_dir, const char *yaml,
                           size_t yaml_len, snaphash_mismatch *first, uint8_t *archive_digest);
/* The two calls above for files whose Blocks carry a BCJ filter in front of LZMA2.  The plain entries answer SNAPHASH_EINVAL
 * for such a file, and keep doing so; these take it when asked to. */
enum { SNAPHASH_UNXZ_BCJ = 1 }; /* accept, Block by Block, the chain of one BCJ filter -- x86 (0x04), ARM (0x07), ARM-Thumb
                                 * (0x08) -- followed by LZMA2, with filter properties of 0 bytes or 4 (the start_offset).
                                 * Every other chain (Delta, PowerPC, IA64, SPARC, two filters in front of LZMA2, ids
                                 * liblzma 5.2.5 does not know) stays SNAPHASH_EINVAL with the plain entries' text.
                                 * SNAPHASH_EFORMAT: properties of any other size, or a start_offset liblzma refuses (not a
                                 * multiple of 4 for ARM, of 2 for Thumb). */
enum { SNAPHASH_UNXZ_CHAINS = 4 }; /* accept, Block by Block, every chain liblzma 5.2.5 reads: up to three
                                    * filters out of Delta (0x03, one property byte: the distance less one), x86, PowerPC
                                    * (0x05), IA64 (0x06), ARM, ARM-Thumb and SPARC (0x09), in any order, repeats allowed, in
                                    * front of LZMA2 -- everything SNAPHASH_UNXZ_BCJ accepts and the rest.  ARM64 (0x0A), RISC-V
                                    * (0x0B) and unknown ids stay SNAPHASH_EINVAL, the text naming the first such filter.
                                    * SNAPHASH_EFORMAT: Delta properties of another size, BCJ properties as above (the
                                    * alignments: 1, 4, 16, 4, 2, 4 for ids 4 .. 9).  Without this flag every answer and every
                                    * text is what it was.  Bit value 2 is not a flag. */
typedef struct snaphash_unxz_options {
    uint32_t struct_size; /* sizeof(snaphash_unxz_options) */
    uint32_t flags;       /* SNAPHASH_UNXZ_*; an unknown bit is SNAPHASH_EINVAL */
} snaphash_unxz_options;
/* opt == NULL, or a struct that is all zero: what snaphash_unxz_buffer / snaphash_tar_unpack_xz do, error text included.
 * With SNAPHASH_UNXZ_BCJ a Block's filter is undone behind its LZMA2 decode and in front of its Check (the Check is over the
 * unfiltered bytes): by the host thread that decoded the Block in the default configuration; under SNAPHASH_FLAG_GPU_ONLY
 * by one launch of the BCJ kernels over the ranges of the Blocks lzma2_blocks_kernel decoded, in front of the Check
 * kernels (Blocks that went to a host thread are filtered there).  snaphash_get_xz_filter_stats tells who did what.  With
 * SNAPHASH_UNXZ_CHAINS a chain of k filters is undone the same way, the filter nearest LZMA2 first: k stages of the filter
 * kernels over the table of Blocks (a Block with a shorter chain is skipped at the later stages); in the stats `filter` is
 * the id a Block's header names first, and a Block counts once however long its chain. */
int snaphash_unxz_buffer_ex(snaphash_ctx *ctx, const void *xz, size_t n, const snaphash_unxz_options *opt, void **out,
                            size_t *out_len);
int snaphash_tar_unpack_xz_ex(snaphash_ctx *ctx, const char *data_tar_xz, const char *target_dir, const char *yaml,
                              size_t yaml_len, const snaphash_unxz_options *opt, snaphash_mismatch *first,
                              uint8_t *archive_digest);
/* The BCJ kernels alone, in place on byte ranges resident in HBM: the twin of snaphash_crc64_device and the tests'
 * instrument.  Range i is d_base[offsets[i] .. + lens[i]) (any alignment, any length; ranges must not overlap) and is
 * filtered as a Block of its own: positions count from its first byte plus start_offset, modulo 2^32.  filter: 4 x86, 7 ARM,
 * 8 ARM-Thumb; encode: nonzero = the producer's direction, 0 = the decoder's.  A range's last 4 bytes (x86), incomplete word
 * (ARM) or halfword pair (Thumb) are left as they are, as liblzma leaves them; the bytes are liblzma's.  SNAPHASH_EINVAL:
 * another filter id, a start_offset that is not a multiple of the filter's alignment (1, 4, 2), more than 2^40 bytes in all.
 * Synchronous; stats.kernel_ms = the kernels (HIP events), stats.launches = their number. */
int snaphash_bcj_device(snaphash_ctx *ctx, uint32_t filter, int encode, void *d_base, const uint64_t *offsets,
                        const uint64_t *lens, size_t n, uint32_t start_offset);
/* The same for every filter liblzma 5.2.5 takes in front of LZMA2: id 3 Delta, 4 x86, 5 PowerPC, 6 IA64,
 * 7 ARM, 8 ARM-Thumb, 9 SPARC.  param: Delta's distance, 1 .. 256 (encode: out[i] = in[i] - in[i - distance], decode its
 * inverse, bytes modulo 256, the bytes in front of a range 0); 0 for every other id.  start_offset: a multiple of the BCJ
 * filter's alignment (1, 4, 16, 4, 2, 4 for ids 4 .. 9); 0 for Delta.  An incomplete last word (PowerPC, SPARC) or 16-byte
 * bundle (IA64) is left as it is.  Delta runs a workgroup a 64 KiB tile of a range, in two launches (encode) or three
 * (decode), none of which waits for another workgroup.  SNAPHASH_EINVAL, touching nothing: any other id (0x0A ARM64 and
 * 0x0B RISC-V among them), a distance of 0 or above 256, a param on a BCJ id, a start_offset off the alignment.  Stats as
 * snaphash_bcj_device's, which is unchanged and keeps to its three ids. */
int snaphash_xz_filter_device(snaphash_ctx *ctx, uint32_t id, uint32_t param, int encode, void *d_base,
                              const uint64_t *offsets, const uint64_t *lens, size_t n, uint32_t start_offset);
/* What the BCJ filters did in the most recent call of this ctx among snaphash_xz_buffer_ex, snaphash_tar_create_xz_ex,
 * snaphash_snap_build with a data.tar.xz, snaphash_unxz_buffer(_ex), snaphash_tar_unpack_xz(_ex) and a .snap session's decode
 * of an .xz member. */
typedef struct snaphash_xz_filter_stats {
    uint32_t struct_size;   /* set by the caller */
    uint32_t filter;        /* the producer's filter; on the install side the filter of the last filtered Block; 0: none */
    uint64_t device_blocks; /* Blocks the BCJ kernels filtered */
    uint64_t host_blocks;   /* Blocks a host thread filtered (install side) */
    double device_ms;       /* the BCJ kernels, HIP events (with the producer's self-check: its undo included) */
} snaphash_xz_filter_stats;
int snaphash_get_xz_filter_stats(const snaphash_ctx *ctx, snaphash_xz_filter_stats *out);
/* One Block of a .xz file by lzma2_blocks_kernel alone, into the caller's HBM: Block `block` (counted over all Streams of
 * xz[0..n), in order) decoded to d_dst[0..dst_len), where dst_len must be the Block's uncompressed size (at most 4 MiB).
 * The container is checked as in snaphash_unxz_buffer; the Block's Check is NOT (snaphash_crc32_device /
 * snaphash_crc64_device / snaphash_sha256_device take it from d_dst).  No byte outside d_dst[0..dst_len) is written.  SNAPHASH_EFORMAT: the
 * kernel refuses the Block's LZMA2 data (no host decoder stands behind this call).  Synchronous. */
int snaphash_unxz_block_device(snaphash_ctx *ctx, const void *xz, size_t n, size_t block, void *d_dst, size_t dst_len);
/* CRC-64/XZ (ECMA-182 reflected, the .xz Check id 4) of byte ranges resident in HBM: the twin of snaphash_crc32_device
 * below, the same rules (a range of length 0 has CRC 0). */
int snaphash_crc64_device(snaphash_ctx *ctx, const void *d_base, const uint64_t *offsets, const uint64_t *lens, size_t n,
                          uint64_t *crcs);
/* SHA-256 (the .xz Check id 10) of byte ranges resident in HBM, by sha256_ranges_kernel: the twin of the call above (any
 * alignment, any length below 32 GiB, ranges may overlap, a range of length 0 has the digest of the empty message);
 * digests: host, n * 32 bytes, each range's at its own index.  A range is one chain on one lane, so many ranges are fast
 * and one long range is not.  Synchronous. */
int snaphash_sha256_device(snaphash_ctx *ctx, const void *d_base, const uint64_t *offsets, const uint64_t *lens, size_t n,
                           uint8_t *digests);

/* Who took the Blocks' Checks in the most recent .xz decode (buffer, tar unpack, or an .xz member of a .snap session, whose
 * snaphash_snap_stats add them up over the session) of this ctx. */
typedef struct snaphash_xz_check_stats {
    uint32_t struct_size;
    uint32_t reserved;
    uint64_t device_crc32, device_crc64, device_sha256; /* Blocks whose Check a kernel took */
    uint64_t host_checks;                               /* Blocks whose Check a host thread took (Check none: counted nowhere) */
    double device_check_ms;                             /* the Check kernels, HIP events */
} snaphash_xz_check_stats;
int snaphash_get_xz_check_stats(const snaphash_ctx *ctx, snaphash_xz_check_stats *out);

/* ---- the .snap itself: the ar container, its two tars, audit and unpack (clickdeb/deb.go:108-203, 408-441) ------------ */

/* CRC-32 of byte ranges resident in HBM (the CRC kernels, crc_kernels.hip; for callers who hold decoded bytes there).
 * kind: 0 = gzip / zlib CRC-32, 1 = bzip2's.  offsets/lens are host arrays; any byte alignment, any length (0: the CRC
 * is 0); ranges may overlap; crcs: host, n values.  Synchronous: the values are there when the call returns. */
int snaphash_crc32_device(snaphash_ctx *ctx, int kind, const void *d_base, const uint64_t *offsets,
                          const uint64_t *lens, size_t n, uint32_t *crcs);

/* A session on one .snap file.  It belongs to ctx and follows its rule (one call in flight; the ctx must outlive it).
 *
 * The container: the global magic "!<arch>\n", 60-byte member headers (name[16], the size in decimal at bytes 48..57,
 * fmag "`\n"), data padded to an even offset.  The reference reads it with an ar library that is not part of its tree,
 * so a member's name is defined HERE: its 16 bytes with trailing spaces removed.  A GNU long-name table ("//") is not
 * supported.  SNAPHASH_EFORMAT: a wrong magic or fmag, a size field that is not digits then spaces, a header or a member
 * the end of the file cuts off.
 * Member lookup is skipToArMember's (deb.go:408-441): the FIRST member whose name starts with "control.tar" /
 * "data.tar" -- a later member of the prefix is never looked at, whatever its suffix; ".gz" takes the gzip engine, ".bz2"
 * the bzip2 engine, and ".xz" snaphash_tar_unpack_xz's engine in a session opened by snaphash_snap_open_ex with
 * SNAPHASH_SNAP_XZ.  In a session opened by snaphash_snap_open ".xz" is, like any other suffix, SNAPHASH_EINVAL with the
 * reference's text "Can not handle NAME" (as snaphash_tar_create answers a name that is not ".gz"): callers and tests rely
 * on that refusal, so the .xz route is asked for.  No member of the prefix is SNAPHASH_EFORMAT with the prefix in the message.
 * An ".xz" member (control.tar.xz as well as data.tar.xz) may be any number of Streams with Stream Padding, Checks none,
 * CRC-32, CRC-64 or SHA-256, every Block LZMA2 alone or one x86, ARM or ARM-Thumb filter in front of LZMA2 -- what
 * SNAPHASH_UNXZ_BCJ takes, what the xz tool the reference pipes the member through reads, and what snaphash_snap_build can
 * write.  Every other chain is SNAPHASH_EINVAL "xz: unsupported filter 0xNN", every other Check id SNAPHASH_EINVAL; like
 * any failed decode it is remembered for that tar, and the other tar stays readable.
 * open reads the file once and decodes nothing.  Each of the two tars is decoded at most once per session, by the
 * first call that needs it; the decoded stream and its member list stay in the session (the reference decodes
 * data.tar.gz once per MetaMember call and once more in Unpack). */
typedef struct snaphash_snap snaphash_snap;
int  snaphash_snap_open(snaphash_ctx *ctx, const char *snap_path, snaphash_snap **out);   /* ClickDeb.Open */
enum { SNAPHASH_SNAP_XZ = 1 }; /* snaphash_snap_open_options.flags: route ".xz" members to the .xz engine (see above) */
enum { SNAPHASH_SNAP_XZ_CHAINS = 4 }; /* with SNAPHASH_SNAP_XZ only (alone: SNAPHASH_EINVAL): ".xz" members may carry every chain
                                       * SNAPHASH_UNXZ_CHAINS takes.  Bit value 2 is not a flag. */
typedef struct snaphash_snap_open_options {
    uint32_t struct_size; /* sizeof(snaphash_snap_open_options) */
    uint32_t flags;       /* SNAPHASH_SNAP_*; an unknown bit is SNAPHASH_EINVAL */
} snaphash_snap_open_options;
/* opt == NULL, or a struct that is all zero: snaphash_snap_open.  Otherwise a struct_size below the struct's is
 * SNAPHASH_EINVAL. */
int  snaphash_snap_open_ex(snaphash_ctx *ctx, const char *snap_path, const snaphash_snap_open_options *opt, snaphash_snap **out);
void snaphash_snap_close(snaphash_snap *s);
size_t snaphash_snap_members(const snaphash_snap *s);
/* name: owned by the session; offset: of the member's data in the file */
int  snaphash_snap_member_info(const snaphash_snap *s, size_t i, const char **name, uint64_t *offset, uint64_t *size);
/* ClickDeb.ControlMember / MetaMember (deb.go:141-183): the LAST tar member with filepath.Clean(hdr.Name) == name
 * ("meta/" joined in front for meta_member); *content malloc'd (snaphash_free), *len 0 and *content NULL when absent */
int  snaphash_snap_control_member(snaphash_snap *s, const char *name, void **content, size_t *len);
int  snaphash_snap_meta_member(snaphash_snap *s, const char *name, void **content, size_t *len);
/* ClickDeb.Unpack (deb.go:188-203) with snaphash_tar_unpack's rules, from the member in memory (no temporary file);
 * verify != 0: also the install-time Verify, against the package's OWN hashes.yaml out of control.tar.* (none there:
 * SNAPHASH_EMISMATCH kind 1, name "hashes.yaml").  archive_digest (may be NULL) and archive-sha512: over the bytes of
 * the data.tar.* member alone.  snaphash_get_unpack_stats then describes the data.tar.* decode of this session. */
int  snaphash_snap_unpack(snaphash_snap *s, const char *target_dir, int verify, snaphash_mismatch *first, uint8_t *archive_digest);
/* Nothing is written: every check the package carries, made on the decoded bytes.  These semantics are this library's
 * (the reference checks nothing of the kind at install time), the first failure in this order:
 *   1. decoding: every gzip member's CRC-32 and ISIZE, every bzip2 block CRC and combined CRC; of an .xz member every
 *      Stream header, every Block header, the CRC-32 of every Index and footer, the Index against its Blocks and every
 *      Block's Check (as snaphash_unxz_buffer); the tar framing: SNAPHASH_EFORMAT (SNAPHASH_ECONTENT for what unpack
 *      would refuse);
 *   2. archive-sha512 against the data.tar.* member's bytes: SNAPHASH_EMISMATCH kind 6;
 *   3. the records of hashes.yaml in yaml order, each against the LAST tar member of its name (names after filepath.Clean,
 *      which drops a leading "./"; an EARLIER member of the name is not looked at, though an unpack would keep the mode
 *      it created the file with): none is kind 1; the type letter or the low nine mode bits of the TAR HEADER differ:
 *      kind 5; for regular files the size: kind 3, then the SHA-512: kind 4;
 *   4. the tar members in tar order: one without a record is kind 2 (the root entry "." is not one).
 * A package without hashes.yaml: kind 1, name "hashes.yaml".  Under SNAPHASH_FLAG_GPU_ONLY the CRCs of (1) are taken by the
 * CRC kernels out of the decoded stream in HBM (a range per gzip member / per bzip2 block; the bzip2 combined CRC is
 * folded from them on the host; a range per .xz Block that lzma2_blocks_kernel decoded, by the CRC-32, CRC-64 or SHA-256
 * kernel its Check names) and the digests by the SHA-512 kernels out of the same buffer; in the default
 * configuration the CRCs stay on host threads.  The verdict is the same in both. */
int  snaphash_snap_audit(snaphash_snap *s, snaphash_mismatch *first, uint8_t *archive_digest);

typedef struct snaphash_snap_stats { /* of the session so far */
    uint32_t struct_size;       /* in: sizeof(snaphash_snap_stats) */
    uint32_t reserved;
    uint64_t data_decodes;      /* times data.tar.* was decoded (at most 1) */
    uint64_t control_decodes;   /* times control.tar.* was decoded (at most 1) */
    uint64_t device_crc_ranges; /* CRCs the CRC kernels took (gzip members, bzip2 blocks, .xz Blocks' Checks of any kind) */
    uint64_t host_crc_ranges;   /* CRCs host threads took (an .xz Block without a Check is counted nowhere) */
    double device_crc_ms;       /* the CRC (for .xz: Check) kernels, HIP events */
} snaphash_snap_stats;
int snaphash_snap_get_stats(const snaphash_snap *s, snaphash_snap_stats *out);

/* ---- writing the .snap: ClickDeb.Build (clickdeb/deb.go:346-406) with snappy.Build's callback (snappy/build.go:269) ---- */

enum { /* snaphash_snap_build_options.flags */
    SNAPHASH_BUILD_NO_HASHES = 1, /* the reference's nil dataTarFinishedCallback: DEBIAN/hashes.yaml is neither computed nor
                                     written (the data member is still hashed for archive_digest) */
    SNAPHASH_BUILD_CHECK = 2      /* "check what you wrote".  With data_codec xz or bz2 the data member is checked by its own
                                     producer's self-check instead (SNAPHASH_XZ_SELF_CHECK / SNAPHASH_BZ2_SELF_CHECK, which
                                     inside the passed options have the same effect for the data member), control.tar.gz
                                     as follows.  The DEFLATE self-check: every 64 KiB chunk of both tars' DEFLATE streams is decoded again in HBM
                                     by deflate_check_kernel and compared with the staged bytes it was made from, before the
                                     bytes travel to the host; a chunk that does not is SNAPHASH_EDEVICE, last_error naming
                                     the member, the chunk and the offset in the tar stream.  It covers the DEFLATE blocks
                                     of every chunk -- not the gzip header and trailer (CRC-32, ISIZE, the final empty block,
                                     written by the host), not the copy back to the host, not the write to disk.  The bytes
                                     written are the same with and without it. */
};

enum { SNAPHASH_DATA_GZ = 0, SNAPHASH_DATA_BZ2 = 1, SNAPHASH_DATA_XZ = 2 }; /* snaphash_snap_build_options.data_codec */

typedef struct snaphash_snap_build_options {
    uint32_t struct_size; /* sizeof(snaphash_snap_build_options); 16 -- the struct before it named a codec -- means gzip */
    uint32_t flags;       /* SNAPHASH_BUILD_* */
    int64_t mtime;        /* of the four ar members, seconds since the epoch; negative = now */
    /* ---- read when struct_size covers them (a struct_size between 16 and the whole struct is SNAPHASH_EINVAL) ---- */
    uint32_t data_codec;  /* SNAPHASH_DATA_*: the member is data.tar.gz, data.tar.bz2 or data.tar.xz; anything else is
                             SNAPHASH_EINVAL.  control.tar.gz stays gzip, as in the reference. */
    uint32_t reserved;    /* must be 0 */
    const snaphash_xz_options *xz;   /* the .xz producer's options as snaphash_tar_create_xz_ex reads them (its refusals and
                                        their texts included); NULL: its defaults.  Not NULL with another codec: SNAPHASH_EINVAL */
    const snaphash_bz2_options *bz2; /* the same for the .bz2 producer and snaphash_tar_create_bz2_ex */
} snaphash_snap_build_options;

typedef struct snaphash_snap_build_stats {
    uint32_t struct_size;   /* in: sizeof(snaphash_snap_build_stats) */
    uint32_t reserved;
    uint64_t snap_bytes;    /* the file written */
    uint64_t data_bytes;    /* its data.tar.* member */
    uint64_t control_bytes; /* its control.tar.gz member */
    uint64_t tar_bytes;     /* the data member's uncompressed tar stream */
    uint64_t members;       /* tar members of the data member */
    uint64_t check_chunks;  /* the self-checks: DEFLATE chunks the check kernel walked (control.tar.gz, and a data.tar.gz), plus
                               the LZMA2 chunks of a data.tar.xz or the bzip2 blocks of a data.tar.bz2, all accepted */
    double check_ms;        /* ... and the checks' kernels' own time, HIP events, summed */
    double data_ms;         /* the fused pass over source_dir (tar, the codec, hashes.yaml, archive digest) */
    double control_ms;      /* the pass over source_dir/DEBIAN */
    double ar_ms;           /* writing the container and hashing it */
    double wall_ms;
} snaphash_snap_build_stats;

/* ClickDeb.Build to the letter, from ONE read of every source file:
 *   data.tar.gz     tarCreate of source_dir without what starts with <source_dir>/DEBIAN (deb.go:361-363), by the fused pass
 *                   of snaphash_tar_create: the member is byte for byte what that call writes for the same tree on the same
 *                   ctx, and the same pass yields hashes.yaml and archive_digest (the SHA-512 of the member);
 *   hashes.yaml     written to <source_dir>/DEBIAN/hashes.yaml, mode 0644, as writeHashes does (snappy/build.go:269) -- the
 *                   dataTarFinishedCallback of snappy.Build; SNAPHASH_BUILD_NO_HASHES writes nothing;
 *   control.tar.gz  tarCreate of <source_dir>/DEBIAN with no exclude rule, through the same producer (no DEBIAN: the walk's
 *                   error, SNAPHASH_EIO);
 *   the container   "!<arch>\n", then debian-binary ("2.0\n"), _click-binary ("0.4\n"), control.tar.gz, data.tar.gz.  The
 *                   reference's ar writer is not part of its tree, so what is written is defined HERE: per member a 60-byte
 *                   header -- the name left-justified in 16 bytes (a longer name: SNAPHASH_EINVAL), the mtime in decimal in
 *                   12, uid "0" and gid "0" in 6 each, the mode in octal in 8 ("100644"), the size in decimal in 10, every
 *                   field padded with spaces, then "`\n" -- the data, and one "\n" after data of odd size (the last
 *                   member's included).  snaphash_snap_open reads back exactly these members.
 * control.tar.gz precedes data.tar.gz and carries the data member's digest, so the data member is written first, to a
 * temporary file beside the target (<snap_path>.data.tar.gz; control likewise), and copied into the container once the control member
 * is known; both temporaries are removed on every way out.  snap_digest (may be NULL): the SHA-512 of the file written, the
 * store's download_sha512, taken while the container is written.  archive_digest (may be NULL): of the data member.
 * opt may be NULL (no flags, mtime now); stats may be NULL.  On failure snap_path is unlinked.
 * With opt->data_codec the data member is written by the .xz or the .bz2 producer instead: data.tar.xz / data.tar.bz2, byte
 * for byte what snaphash_tar_create_xz_ex / snaphash_tar_create_bz2_ex write for the same tree with exclude_prefix
 * <source_dir>/DEBIAN and the same options on the same ctx, from the same single pass that yields hashes.yaml and
 * archive_digest; the temporary is <snap_path>.data.tar.xz / .bz2 and the ar member has that name (snaphash_snap_open_ex with
 * SNAPHASH_SNAP_XZ reads a data.tar.xz back).  A chunk or block the member's self-check refuses fails the build with the
 * producer's error.  snaphash_get_xz_selfcheck_stats, snaphash_get_xz_filter_stats and snaphash_get_bz2_selfcheck_stats then
 * describe the data member.  With opt == NULL or a struct_size of 16 the file is what it always was. */
int snaphash_snap_build(snaphash_ctx *ctx, const char *source_dir, const char *snap_path, const snaphash_snap_build_options *opt,
                        uint8_t *archive_digest, uint8_t *snap_digest, snaphash_snap_build_stats *stats);

typedef struct snaphash_deflate_verdict {
    uint32_t status; /* 0 accepted; 1 a literal or stored byte differs; 2 a match's copy differs; 3 a distance beyond
                        min(32768, bytes in front); 4 not RFC 1951 (or BFINAL before the last chunk); 5 the blocks produce more
                        than the chunk; 6 they end at the stretch's end with fewer; 7 they do not end at the stretch's end;
                        8 the chunk's table entry lies outside the compressed bytes */
    uint32_t offset; /* within the chunk: the first byte that differs, else how far the walk had come */
} snaphash_deflate_verdict;
/* The self-check kernel alone, on tables the caller wrote (tests): d_in[0..n_in) is the staged stream in HBM, cut into
 * nchunks chunks of 65 536 bytes (nchunks * 65 536 >= n_in; a chunk past the end is empty); d_z holds z_off[nchunks] compressed
 * bytes, chunk c's stretch being [z_off[c], z_off[c + 1]) (host array of nchunks + 1 ascending offsets).  A chunk is accepted
 * when its stretch is a sequence of RFC 1951 blocks -- any valid one -- that produces exactly the chunk's bytes, matches
 * reaching at most min(32768, bytes of d_in in front of them) back, and ends exactly at the stretch's end: without BFINAL
 * on a byte boundary (after an empty stored block, or a stored chunk), or -- last_is_final != 0, last chunk only -- with
 * the byte after the final block.  verdicts: nchunks entries (host).  Nothing is written to HBM but the verdicts, in a
 * buffer of the library's own.  SNAPHASH_EINVAL: a null pointer, nchunks == 0 or too few for n_in, offsets that descend.
 * Synchronous. */
int snaphash_deflate_check_device(snaphash_ctx *ctx, const void *d_in, size_t n_in, const void *d_z, const uint64_t *z_off,
                                  size_t nchunks, int last_is_final, snaphash_deflate_verdict *verdicts);

/* ---- neighbouring scan: helpers.FilesAreEqual / DirUpdated -------- */

/* helpers.FilesAreEqual (helpers/cmp.go:31-60), batched: equal[i] = 1 iff a[i] and b[i] both
 * open, have the same size and the same bytes; as upstream, any open/stat/read error makes the
 * pair "not equal" (it is not an error of the call).  The bytes are compared on the GPU; a ctx with several
 * devices deals the pairs to its engines (LPT by size), each over its own PCIe link. */
int snaphash_files_equal(snaphash_ctx *ctx, const char *const *a, const char *const *b, size_t n,
                         uint8_t *equal);

/* The same for byte ranges already resident in HBM: [d_a+off_a[i], +lens[i]) against
 * [d_b+off_b[i], +lens[i]).  Offsets (host arrays) and bases 16-byte aligned; d_equal is device
 * memory, n bytes.  The kernel reads the whole 16-byte piece that holds a range's last byte: on
 * both sides the bytes up to the next 16-byte boundary must be readable; their values are ignored.
 * Enqueues on the ctx stream; snaphash_sync waits.  HBM-bound: 2 bytes read per byte compared. */
int snaphash_ranges_equal_device(snaphash_ctx *ctx, const void *d_a, const uint64_t *off_a,
                                 const void *d_b, const uint64_t *off_b, const uint64_t *lens,
                                 size_t n, void *d_equal);

/* helpers.DirUpdated (helpers/cmp.go:88-114): the non-directory entries of dir_a (Glob order)
 * that also exist in dir_b and differ from them, each with pfx prepended.  *names_out is a
 * malloc'd sequence of *count NUL-terminated strings laid end to end (snaphash_free). */
int snaphash_dir_updated(snaphash_ctx *ctx, const char *dir_a, const char *dir_b, const char *pfx,
                         char **names_out, size_t *count);

/* ---- host-side pieces of the pass (no device needed) ----------------------- */

typedef struct snaphash_records snaphash_records;
typedef struct snaphash_record {
    const char *name;  /* relative to the walk root, '/' separated; owned by the record set */
    uint32_t st_mode;  /* lstat st_mode */
    int32_t is_regular;
    int64_t size;      /* valid when is_regular */
    const char *path;  /* root-joined path; owned by the record set */
} snaphash_record;

/* filepath.Walk exactly as writeHashes uses it (build.go:228-259): pre-order,
 * children byte-wise sorted per directory, lstat, "/DEBIAN" string-prefix skip,
 * root skipped. */
int snaphash_walk(const char *build_dir, snaphash_records **out);
size_t snaphash_records_count(const snaphash_records *r);
int snaphash_records_get(const snaphash_records *r, size_t i, snaphash_record *out);
void snaphash_records_free(snaphash_records *r);

/* yaml.Marshal(hashesYaml) for the records (hashes.go:93-110).  file_digests
 * holds one raw 64-byte digest per REGULAR record, in record order. */
int snaphash_emit_yaml(const snaphash_records *r, const uint8_t archive_digest[64],
                       const uint8_t *file_digests, char **yaml_out, size_t *yaml_len);

/* yaml.Unmarshal into hashesYaml (the reader side, snappy/snapp.go:466-478): parses the
 * yaml.v2 rendering of the schema -- plain, 'single' and "double" quoted scalars, the
 * empty document {} (common_test.go:77-80), files: [] -- into a record set (path is "",
 * st_mode carries type + permission bits).  archive_hex (may be NULL) receives
 * archive-sha512 as written, NUL-terminated, at most 128 characters. */
int snaphash_parse_yaml(const char *yaml, size_t yaml_len, snaphash_records **out, char archive_hex[129]);
/* sha512 hexdigest text of record i of a parsed set ("" for directories, symlinks and
 * for record sets that come from snaphash_walk). */
const char *snaphash_records_sha512_hex(const snaphash_records *r, size_t i);

/* yamlFileMode.MarshalYAML / UnmarshalYAML (hashes.go:33-88).  out: 11 bytes.
 * mode_parse yields a POSIX st_mode (S_IFDIR/S_IFLNK/S_IFREG | perm bits) and
 * rejects the empty string instead of indexing it. */
int snaphash_mode_string(uint32_t st_mode, char out[11]);
int snaphash_mode_parse(const char *s, uint32_t *st_mode);

/* Longest-processing-time shard assignment of n files (by SHA-512 block count)
 * to nshards GPUs; shard_of[i] in [0,nshards).  Deterministic. */
int snaphash_lpt_assign(const uint64_t *lens, size_t n, int nshards, int32_t *shard_of);

/* Deterministic synthetic content (SURVEY sec. 8d generator), written straight
 * into HBM; offsets/lens/file_index are host arrays.  Benchmark/test utility. */
int snaphash_fill_synthetic_device(snaphash_ctx *ctx, void *d_base, const uint64_t *offsets,
                                   const uint64_t *lens, const uint64_t *file_index, size_t n);

/* ---- diagnostics ------------------------------------------------------------ */
const char *snaphash_strerror(int code);
const char *snaphash_last_error(const snaphash_ctx *ctx); /* ctx == NULL: why the last snaphash_init on this thread failed */
void snaphash_get_stats(const snaphash_ctx *ctx, snaphash_stats *out); /* several devices: sums; the *_ms are the slowest device's */
int snaphash_get_stats_ex(const snaphash_ctx *ctx, snaphash_stats_ex *out);
/* per engine i < n_devices: its HIP ordinal and its own stats of the most recent call */
int snaphash_get_device_stats(const snaphash_ctx *ctx, uint32_t i, int32_t *device, snaphash_stats *out);

/* ---- ABI 3: where an engine's staging lives -------------------------------------------------------------
 * One engine per GPU moves ~55 GB/s over its own PCIe link; on a two-socket node the pinned staging buffers and
 * the threads that fill them belong on the socket the GPU hangs off.  snaphash_init reads the GPU's NUMA node
 * from sysfs (/sys/bus/pci/devices/<bdf>/numa_node), allocates the engine's pinned memory there and binds the
 * engine's fill threads to that node's CPUs; a ctx with several engines divides the CPUs it may use among them.
 * Nothing in the reference corresponds to this (its pass is one goroutine, snappy/build.go:228). */
typedef struct snaphash_engine_info {
    uint32_t struct_size;  /* in: sizeof(snaphash_engine_info) */
    int32_t device;        /* HIP ordinal */
    int32_t numa_node;     /* the GPU's node as sysfs reports it; -1 = unknown, single-node host or SNAPHASH_FLAG_NO_NUMA */
    int32_t staging_node;  /* node the engine's first pinned staging page was found on; -1 = not allocated yet / unknown */
    uint32_t fill_threads; /* most staging-fill threads the engine uses at a time */
    uint32_t n_cpus;       /* CPUs of numa_node the fill threads are bound to (0 = not bound) */
    char pci_bus_id[32];
    /* ---- ABI 4 (filled when struct_size covers them; an ABI 3 caller's shorter struct is still accepted) ---- */
    uint64_t pinned_bytes; /* pinned host memory the engine holds right now (staging slots, job arrays, comparison tables, DEFLATE,
                            * inflate and bzip2 scratch) */
    uint64_t hbm_bytes;    /* device memory it holds (staging slots, job arrays, chaining values, digests, comparison tables,
                            * DEFLATE, inflate and bzip2 scratch including the decoded stream, gather buffer) */
} snaphash_engine_info;
int snaphash_get_engine_info(const snaphash_ctx *ctx, uint32_t i, snaphash_engine_info *out);
/* The CPUs engine i's fill threads are bound to (ABI 4): engines on one NUMA node get disjoint slices of its CPUs (whole
 * cores: a slice of every SMT sibling run).  *n_cpus = how many; cpus (may be NULL) receives up to cap of them. */
int snaphash_get_engine_cpus(const snaphash_ctx *ctx, uint32_t i, int32_t *cpus, size_t cap, size_t *n_cpus);

/* ---- ABI 4: the plan of a call, host-only (no device needed) ------------------------------------------------
 * What the planner (snaphash_config.host_threads) decides for n streams of the given lengths under a cost model;
 * on_host[i] = 1: a host thread hashes stream i.  Zeros in the model = the library's measured MI355X defaults.
 * The entry points plan with the ctx's own numbers (cores and host rate measured at snaphash_init). */
typedef struct snaphash_plan_model {
    uint32_t struct_size;    /* in: sizeof(snaphash_plan_model) */
    uint32_t n_devices;      /* engines the GPU part is sharded over (0 = 1) */
    uint32_t cpus;           /* host cores the call may keep busy (0 = what this process may use) */
    uint32_t fill_threads;   /* cores one engine's staging fill occupies beside a GPU part (0 = 6 for memory, 12 for files) */
    uint32_t host_threads;   /* 0 = automatic, N = exactly N (as snaphash_config.host_threads) */
    uint32_t from_files;     /* sources are paths rather than caller memory */
    double host_rate;        /* B/s, one host core's SHA-512 (0 = 1.4e9) */
    double gpu_stream_rate;  /* B/s, ONE stream under the lane-pair kernel (0 = 44e6) */
    double gpu_link;         /* B/s, one engine's staging + PCIe copy (0 = 55e9 memory, 54e9 files) */
    double gpu_latency;      /* s per launch whatever its size (0 = 150e-6) */
    /* out */
    double gpu_seconds;      /* modelled makespan of the GPU part (0 = none) */
    double host_seconds;     /* modelled makespan of the host part */
    uint64_t host_streams, host_bytes;
    uint32_t host_threads_used;
    uint32_t host_lane_gain_pct; /* IN (was reserved, 0): what a host thread gains from running its streams eight at a time, a
                                    stream per AVX-512 lane, in percent of its one-stream rate; 0 or 100 = none.  A ctx plans with
                                    240 for files and 320 for memory where the CPU has AVX-512F/BW (snaphash_get_plan_model
                                    returns what it uses). */
    /* ---- ABI 5 (read when struct_size covers it) ---- */
    double fill_rate;        /* IN: B/s ONE staging-fill thread moves (0 = 9e9 from memory, 6.5e9 pread of files) */
    double fill_per_file;    /* IN: s a stream costs a fill thread whatever its length -- for files the open and close beside the other
                                threads' (0 = 10e-6 files, 0.3e-6 memory) */
} snaphash_plan_model;
int snaphash_plan_streams(const uint64_t *lens, size_t n, snaphash_plan_model *model /* in/out */, uint8_t *on_host /* n, may be NULL */);
/* ABI 5: the model `ctx` plans a call with right now -- cores, threads, the host rate measured at init, and the link and
 * fill rates as calibrated on this box so far (at init, then by every staged call) -- so that snaphash_plan_streams
 * reproduces the ctx's own plan.  model->struct_size in; the out fields are zeroed. */
int snaphash_get_plan_model(const snaphash_ctx *ctx, int from_files, snaphash_plan_model *model);
/* ABI 5, host-only: the calibration's update rule by itself (what a ctx applies after each staged call): an observation
 * of `bytes` moved in `seconds` -- what = 0: an engine's H2D copies (HIP event time), 1: one fill thread from memory,
 * 2: one fill thread preading files (wall x threads); 3 / 4: a call that went to host threads whole measured no fill from
 * memory / files, and the estimate moves a quarter of the way back to the model's default (bytes and seconds unused);
 * 5: a host part planned at `bytes` SECONDS took `seconds` (busiest thread): the host rate's correction, 0.6 .. 1.6;
 * 6: the fill threads spent `seconds` (wall x threads, less what the bytes took at the fill rate) on `bytes` FILES of a
 * call of small files: what a file costs a fill thread beside the others (open, close), 0.3 .. 2 x the default 10 us.
 * Returns 1 when the observation was taken, 0 when it was too small or implausible to mean anything, negative on bad
 * arguments.  How far an observation is believed: the link within a factor of four of the defaults' 56.7 GB/s, a fill
 * thread down to half of its default and never above it (planner.h).  snaphash_calib_apply writes the calibrated
 * gpu_link / fill_rate / fill_per_file into a model that has not set them (from_files decides which) and corrects its
 * host_rate (1.4e9 where it names none) by what host parts took.
 * What a ctx observes of a call: the link only from calls whose copies average 32 MiB or more (a small copy measures
 * its latency), the fill rate only from calls whose streams average 256 KiB or more and net of the per-file cost, the
 * per-file cost only from calls of 256 files or more that average under 64 KiB. */
typedef struct snaphash_plan_calib {
    uint32_t struct_size; /* in: sizeof(snaphash_plan_calib) */
    uint32_t n_dma, n_fill_mem, n_fill_files; /* observations taken */
    double dma;           /* B/s, 0 = not measured */
    double fill_mem, fill_files;
    double host_gain;     /* what host threads really did over what the model said (x the model's host rate); 0 = not measured */
    uint32_t n_host, n_fill_per_file;
    double fill_per_file; /* s per file on a fill thread; 0 = not measured */
} snaphash_plan_calib;
int snaphash_calib_observe(snaphash_plan_calib *calib, int what, double bytes, double seconds);
/* One staged call of an engine, sorted into those observations by what it can speak about (the rule above; what a ctx does
 * after every staged call): `bytes` of `streams` streams went over the link in `copies` copies taking `h2d_seconds`, the fill
 * threads spent `fill_thread_seconds` (wall x threads) on them. */
int snaphash_calib_observe_call(snaphash_plan_calib *calib, int from_files, double bytes, double streams, double copies,
                                double h2d_seconds, double fill_thread_seconds);
int snaphash_calib_apply(const snaphash_plan_calib *calib, snaphash_plan_model *model);
int snaphash_get_calib(const snaphash_ctx *ctx, snaphash_plan_calib *out); /* what ctx has measured so far */
/* CPUs this process may keep busy: affinity mask capped by the cgroup CPU quota (what host_threads = 0 plans with). */
uint32_t snaphash_usable_cpus(void);
/* the quota part alone, on any cgroup tree (tests): whole CPUs, 0 = none found */
uint32_t snaphash_cgroup_cpu_quota(const char *cgroup_root, const char *proc_self_cgroup);

/* ---- ABI 4: the pass with one process per GPU (SURVEY sec. 8e as torch.distributed / MPI launch it) -----------------
 * writeHashes (build.go:216-270) over `world` ranks, each with its own ctx on its own GPU: every rank calls
 * snaphash_shard_plan with the same tree (the walk and the LPT plan by SHA-512 block count are deterministic; the
 * archive is stream 0, as in the Go batch shape), hashes ITS members with snaphash_shard_hash into a slab of
 * snaphash_shard_rows() x 64 bytes (unused rows zero), the caller all-gathers the slabs in rank order (RCCL:
 * torch.distributed.all_gather_into_tensor or ncclAllGather), and any rank turns world x rows x 64 bytes into
 * hashes.yaml with snaphash_shard_emit (malloc'd; snaphash_free).  plan and emit need no device.  The one-process form
 * of the same thing is snaphash_config.devices.  snaphash_shard_hash plans and fills with the rank's SHARE of the cores
 * this process may use, the allowance over the ranks on THIS node: eight ranks on a node do not each claim all of it.
 * How many ranks share the node comes from the caller -- snaphash_shard_set_local_ranks (ABI 5), else the launcher's
 * LOCAL_WORLD_SIZE (torch.distributed.run, mpirun's OMPI_COMM_WORLD_LOCAL_SIZE) -- and only without either from
 * min(world, visible GPUs), which is wrong under a launcher that shows every rank ONE device.
 * Every rank must have walked the SAME tree: snaphash_shard_fingerprint (ABI 5) is a 64-bit hash of the plan (names,
 * sizes, modes, who hashes what) for the caller to compare across ranks BEFORE the all-gather -- a tree that changed
 * between two ranks' walks otherwise ends in mismatched slabs or a hung collective (snappy_amd/sharded.py does it). */
/* A shard handle is used by one thread at a time (snaphash_shard_emit joins the thread that has been writing the
 * document since the plan). */
typedef struct snaphash_shard snaphash_shard;
int snaphash_shard_plan(const char *build_dir, const char *data_tar, uint32_t rank, uint32_t world, snaphash_shard **out);
size_t snaphash_shard_rows(const snaphash_shard *sh);     /* rows of every rank's slab */
size_t snaphash_shard_count(const snaphash_shard *sh);    /* streams this rank hashes */
size_t snaphash_shard_streams(const snaphash_shard *sh);  /* streams of the whole job (1 + regular files) */
uint64_t snaphash_shard_bytes(const snaphash_shard *sh);  /* bytes this rank hashes */
const char *snaphash_shard_path(const snaphash_shard *sh, size_t k); /* k-th stream of this rank, in slab row order */
int snaphash_shard_hash(snaphash_ctx *ctx, snaphash_shard *sh, uint8_t *slab /* rows * 64, host */);
int snaphash_shard_emit(const snaphash_shard *sh, const uint8_t *slabs /* world * rows * 64, rank-major */,
                        char **yaml_out, size_t *yaml_len);
void snaphash_shard_free(snaphash_shard *sh);
/* ABI 5: the ranks SHARE the walk.  snaphash_shard_plan has every rank walk the whole tree (every Lstat issued `world`
 * times over).  Instead: every rank calls snaphash_shard_list -- it lists the root, walks the subtrees of the root's
 * entries i with i mod world == rank and returns what it found as a blob (malloc'd; snaphash_free) -- the caller
 * all-gathers the blobs (their lengths first), and every rank calls snaphash_shard_plan_from with all `world` blobs in
 * rank order: the record list is rebuilt from them in filepath.Walk's order, identical on every rank, and the handle is
 * what snaphash_shard_plan would have returned (same fingerprint).  SNAPHASH_EMISMATCH: the ranks listed different roots.
 * A tree whose files all sit directly in the root gains nothing (the root's entries are dealt out, not its files' bytes). */
int snaphash_shard_list(const char *build_dir, uint32_t rank, uint32_t world, void **blob_out, size_t *blob_len);
int snaphash_shard_plan_from(const char *build_dir, const char *data_tar, uint32_t rank, uint32_t world,
                             const void *const *blobs, const size_t *blob_lens, snaphash_shard **out);
int snaphash_shard_set_local_ranks(snaphash_shard *sh, uint32_t ranks_on_this_node /* 0 = as found (see above) */);
uint64_t snaphash_shard_fingerprint(const snaphash_shard *sh);

/* Host-only: the topology probe the engines use, on any sysfs tree (the tests hand in a fake one).  *node = NUMA node
 * of the PCI function (-1 unknown); cpus (may be NULL) receives up to cap CPU numbers of that node, *n_cpus how many
 * the node has. */
int snaphash_numa_probe(const char *sysfs_root, const char *pci_bus_id, int32_t *node, int32_t *cpus, size_t cap,
                        size_t *n_cpus);
/* Host-only (ABI 4): the CPUs engine `pos` of the `m` engines on NUMA node `node` gets (snaphash_get_engine_cpus on a
 * live ctx): slice pos of every contiguous run of the node's cpulist. */
int snaphash_numa_slice(const char *sysfs_root, int32_t node, uint32_t pos, uint32_t m, int32_t *cpus, size_t cap,
                        size_t *n_cpus);

#ifdef __cplusplus
}
#endif
#endif /* SNAPHASH_H */
