/* snaphash -- command-line front end of libsnaphash.so for non-Go callers.
 *   snaphash [options] hash FILE...              sha512sum-style lines (helpers.Sha512sum, batched)
 *   snaphash [options] tree BUILD_DIR DATA_TAR   hashes.yaml on stdout (writeHashes minus the file write)
 *   snaphash [options] write BUILD_DIR DATA_TAR  writeHashes: BUILD_DIR/DEBIAN/hashes.yaml
 *   snaphash [options] verify DIR YAML [TAR]     re-hash DIR against a hashes.yaml; exit 1 on mismatch
 *   snaphash [options] build BUILD_DIR OUT.tar.gz
 *                                      Build's data step fused (clickdeb/deb.go:261-344 + snappy/build.go:517-520):
 *                                      data.tar.gz of BUILD_DIR without DEBIAN/, every file read once, then
 *                                      BUILD_DIR/DEBIAN/hashes.yaml with the archive's digest
 *   snaphash [options] build-xz [-c] [-B KiB] [-C none|crc32|crc64|sha256] [-F FILTERS] [-L 0|1] BUILD_DIR OUT.tar.xz
 *                                      the same with data.tar.xz (tarCreate's ".xz" branch): Blocks of 1 MiB (or -B), Check
 *                                      CRC-64 (or -C), LZMA2 on the GPU; -c: the LZMA2 self-check on the GPU; -F: a BCJ
 *                                      filter in front of LZMA2, applied on the GPU (what xz writes when XZ_OPT names one)
 *   snaphash [options] build-bz2 [-c] [-L LEVEL] BUILD_DIR OUT.tar.bz2
 *                                      the same with data.tar.bz2 (level 9, or -L): every bzip2 block coded on the GPU; -c: every
 *                                      block decoded again and compared on the GPU (the .bz2 self-check)
 *   snaphash [options] gzip IN OUT.gz            the compressor alone, one gzip member
 *   snaphash [options] bzip2 [-L LEVEL] [-c] IN OUT.bz2   the bzip2 compressor alone, level 1..9 (default 9); -c: the .bz2
 *                                                self-check on the GPU (-s prints what it checked)
 *   snaphash [options] xz IN OUT.xz [-B KiB] [-C none|crc32|crc64|sha256] [-c] [-F FILTERS] [-L 0|1]
 *                                                the .xz compressor alone, a Block per KiB of input (default 1024), the
 *                                                Blocks' Check as named (default crc64), taken on the GPU; -c: the LZMA2
 *                                                self-check on the GPU (-s prints what it walked); -F: a BCJ filter
 *                                                in front of LZMA2 (-s prints what the filter kernels did)
 *   snaphash [options] gunzip IN.gz OUT          the inverse: every member decoded (GPU inflate)
 *   snaphash [options] unpack DATA_TAR_GZ DIR [HASHES_YAML]
 *   snaphash [options] bunzip2 IN.bz2 OUT        every bzip2 stream decoded (blocks side by side)
 *   snaphash [options] unpack-bz2 DATA_TAR_BZ2 DIR [HASHES_YAML]
 *   snaphash [options] unxz [-F|-A] IN.xz OUT    every .xz Stream decoded (Blocks side by side); -F: Blocks with an x86, ARM
 *                                                or ARM-Thumb filter in front of LZMA2 are taken too (SNAPHASH_UNXZ_BCJ);
 *                                                -A: Blocks with any chain liblzma reads (SNAPHASH_UNXZ_CHAINS)
 *   snaphash [options] unpack-xz [-F|-A] DATA_TAR_XZ DIR [HASHES_YAML]
 *                                      ClickDeb.Unpack (clickdeb/deb.go:188-203) into DIR; with HASHES_YAML also the
 *                                      install-time Verify from the decoded bytes; exit 1 on mismatch
 *   snaphash [options] snap ls FILE.snap         the ar members of the package: size, offset, name
 *   snaphash [options] snap cat-control NAME FILE.snap   ClickDeb.ControlMember on stdout (exit 1 when absent)
 *   snaphash [options] snap cat-meta NAME FILE.snap      ClickDeb.MetaMember on stdout (exit 1 when absent)
 *   snaphash [options] snap audit FILE.snap      every check the package carries, nothing written; exit 1 on mismatch
 *   snaphash [options] snap unpack DIR FILE.snap ClickDeb.Unpack + Verify against the package's own hashes.yaml;
 *                                      exit 1 on mismatch; -s prints the unpack and session statistics
 *   snaphash [options] snap -x VERB ...          the five verbs above on a package with control.tar.xz / data.tar.xz members
 *                                      (SNAPHASH_SNAP_XZ); without -x such a member is "Can not handle NAME"; -x -A: their
 *                                      Blocks may carry any filter chain (SNAPHASH_SNAP_XZ_CHAINS)
 *   FILTERS (-F of build-xz, xz, snap build): x86 | arm | armthumb (the `filter` field), or a comma list of up to three of
 *                                      delta:N (N = 1 .. 256), x86, powerpc, ia64, arm, armthumb, sparc: the chain in front of
 *                                      LZMA2, the Block header's first filter first
 *   snaphash [options] snap build [-c] [-Z gz|xz|bz2] [-L LEVEL] [-F FILTERS] [-C none|crc32|crc64|sha256] [-B KiB] DIR OUT.snap
 *                                      ClickDeb.Build with writeHashes fused in: DIR (with its DEBIAN/) -> the
 *                                      package, DIR/DEBIAN/hashes.yaml written on the way; prints the SHA-512 of the file
 *                                      (the store's download_sha512); -c: the self-checks on the GPU; -Z: the data member's
 *                                      codec (default gz, what the reference writes), -L -F -C -B as build-xz and build-bz2
 *                                      take them for that codec; -s names the member written
 *   snaphash [options] cmp A B [A B ...]         helpers.FilesAreEqual per pair; exit 1 if any pair differs
 *   snaphash [options] dirupdated DIR_A DIR_B [PREFIX]   helpers.DirUpdated
 * options: -d DEV[,DEV...]  engines (default: the current device; -1 = all visible)
 *          -t N             hybrid scheduling: oversize streams finish on N host threads
 *          -b               gunzip / unpack: also cut streams without flush points at their DEFLATE blocks
 *                           (SNAPHASH_FLAG_SPLIT_BLOCKS); -s then prints the block scan's statistics too
 *          -s               print the statistics of the call on stderr
 * without -d/-t the environment may name them: SNAPHASH_DEVICES=all|0,1,...  SNAPHASH_HOST_THREADS=N
 * Pure C against include/snaphash.h: it is also the smallest example of the ABI. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "../../include/snaphash.h"

static int die(snaphash_ctx *c, int rc, const char *what)
{
    fprintf(stderr, "snaphash: %s: %s (%s)\n", what, snaphash_strerror(rc), snaphash_last_error(c)); /* c == NULL: why snaphash_init failed */
    return rc == SNAPHASH_EMISMATCH ? 1 : 2;
}

static int usage(void)
{
    fprintf(stderr, "usage: snaphash [-d DEV,...] [-t HOST_THREADS] [-g] [-b] [-z DEPTH] [-s] hash FILE... | tree DIR TAR | write DIR TAR |\n"
                    "       verify DIR YAML [TAR] | build DIR OUT.tar.gz | gzip IN OUT.gz | gunzip IN.gz OUT |\n"
                    "       build-xz [-c] [-B BLOCK_KiB] [-C none|crc32|crc64|sha256] [-F FILTERS] [-L 0|1] DIR OUT.tar.xz |\n"
                    "       build-bz2 DIR OUT.tar.bz2 | bzip2 [-L LEVEL] IN OUT.bz2 |\n"
                    "       (in front of their names build-bz2 also takes [-c] [-L LEVEL] and bzip2 [-c]: -c is the .bz2 self-check)\n"
                    "       xz IN OUT.xz [-B BLOCK_KiB] [-C none|crc32|crc64|sha256] [-c] [-F FILTERS] [-L 0|1] |\n"
                    "       unpack DATA_TAR_GZ DIR [HASHES_YAML] | bunzip2 IN.bz2 OUT |\n"
                    "       unpack-bz2 DATA_TAR_BZ2 DIR [HASHES_YAML] | unxz [-F] IN.xz OUT |\n"
                    "       unpack-xz [-F] DATA_TAR_XZ DIR [HASHES_YAML] | cmp A B [A B ...] |\n"
                    "       (-F on the two .xz decoding commands: also take Blocks with a BCJ filter in front of LZMA2; -A: with any chain)\n"
                    "       (FILTERS: x86 | arm | armthumb, or a comma list of up to three of delta:N powerpc ia64 sparc and those)\n"
                    "       (snap -x -A VERB: .xz members with any filter chain)\n"
                    "       snap [-x] {ls | cat-control NAME | cat-meta NAME | audit | unpack DIR} FILE.snap  (-x: .xz members are read too) |\n"
                    "       snap build [-c] [-Z gz|xz|bz2] [-L LEVEL] [-F FILTERS] [-C none|crc32|crc64|sha256] [-B BLOCK_KiB] DIR OUT.snap |\n"
                    "       dirupdated DIR_A DIR_B [PREFIX] | plan FILE... (what the planner would do; no device needed)\n"
                    "       -g: every byte through the HIP kernels (SNAPHASH_FLAG_GPU_ONLY); default: every call is planned\n"
                    "       -b: gunzip / unpack also split streams without flush points at their blocks (SNAPHASH_FLAG_SPLIT_BLOCKS)\n"
                    "       -z DEPTH: effort of `build` / `gzip` (hash-chain links per position; default 96 = gzip -9's bytes, 32 = gzip -6's)\n");
    return 2;
}

/* -b -s: what the block scan and the link did in the last gunzip / unpack */
static void print_block_stats(snaphash_ctx *c, const char *what)
{
    snaphash_block_scan_stats b;
    b.struct_size = sizeof b;
    if (!snaphash_get_block_scan_stats(c, &b))
        fprintf(stderr, "%s: block scan: %llu bit offsets, %llu candidates, %llu segments linked from them, %llu unreached, "
                        "%llu host stretches, scan %.2f ms\n",
                what, (unsigned long long)b.bits_scanned, (unsigned long long)b.candidates, (unsigned long long)b.linked,
                (unsigned long long)b.unreached, (unsigned long long)b.host_blocks, b.scan_ms);
}

/* -C's word -> the Check id, or -1 */
static int xz_check_id(const char *w)
{
    return !strcmp(w, "none") ? 0 : !strcmp(w, "crc32") ? 1 : !strcmp(w, "crc64") ? 4 : !strcmp(w, "sha256") ? 10 : -1;
}

/* -F's word -> the filter id, or 0 */
static uint32_t xz_filter_id(const char *w)
{
    return !strcmp(w, "x86") ? 4u : !strcmp(w, "arm") ? 7u : (!strcmp(w, "armthumb") || !strcmp(w, "thumb")) ? 8u : 0u;
}

/* -F's word into the options: one of x86 / arm / armthumb sets `filter`, as it always did; anything else is a comma list of up
 * to three of delta:N (N = 1 .. 256), x86, powerpc, ia64, arm, armthumb, sparc and sets the chain.  0: not such a word */
static int xz_filter_arg(const char *w, snaphash_xz_options *xo)
{
    if ((xo->filter = xz_filter_id(w)) != 0) return 1;
    uint32_t n = 0;
    while (*w) {
        char word[16];
        size_t len = strcspn(w, ",");
        if (len == 0 || len >= sizeof word || n == 3) return 0;
        memcpy(word, w, len);
        word[len] = 0;
        uint32_t id = xz_filter_id(word), param = 0;
        if (!id) id = !strcmp(word, "powerpc") ? 5u : !strcmp(word, "ia64") ? 6u : !strcmp(word, "sparc") ? 9u : 0u;
        if (!id && !strncmp(word, "delta:", 6)) {
            char *end = NULL;
            const unsigned long d = strtoul(word + 6, &end, 10);
            if (!word[6] || *end || d < 1 || d > 256) return 0;
            id = 3;
            param = (uint32_t)d;
        }
        if (!id) return 0;
        xo->chain[n++] = id | param << 8;
        w += len;
        if (*w == ',') {
            if (!w[1]) return 0;
            w++;
        }
    }
    xo->chain_len = n;
    return n != 0;
}

/* the .xz commands' -L: the level, 0 or 1, or -1 */
static int xz_level(const char *w)
{
    return !strcmp(w, "0") ? 0 : !strcmp(w, "1") ? 1 : -1;
}

/* -s after an .xz call with -F: what the BCJ filters did */
static void print_xz_filter(snaphash_ctx *c, const char *what)
{
    snaphash_xz_filter_stats s;
    s.struct_size = sizeof s;
    if (!snaphash_get_xz_filter_stats(c, &s))
        fprintf(stderr, "%s: filter 0x%02X: %llu blocks on the GPU (%.3f ms), %llu on host threads\n", what, s.filter,
                (unsigned long long)s.device_blocks, s.device_ms, (unsigned long long)s.host_blocks);
}

/* -s after an .xz producer call with -c: what the self-check walked */
static void print_xz_selfcheck(snaphash_ctx *c, const char *what)
{
    snaphash_xz_selfcheck_stats s;
    s.struct_size = sizeof s;
    if (!snaphash_get_xz_selfcheck_stats(c, &s))
        fprintf(stderr, "%s: self-check: %llu chunks, %.3f ms\n", what, (unsigned long long)s.chunks, s.ms);
}

/* -s after a .bz2 producer call with -c: what the self-check decoded again */
static void print_bz2_selfcheck(snaphash_ctx *c, const char *what)
{
    snaphash_bz2_selfcheck_stats s;
    s.struct_size = sizeof s;
    if (!snaphash_get_bz2_selfcheck_stats(c, &s))
        fprintf(stderr, "%s: self-check: %llu blocks, %.3f ms\n", what, (unsigned long long)s.blocks, s.ms);
}

/* -L's word -> the level 1..9, or 0 */
static unsigned bz2_level(const char *w)
{
    return (w[0] >= '1' && w[0] <= '9' && !w[1]) ? (unsigned)(w[0] - '0') : 0;
}

static char *slurp(const char *path, size_t *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return NULL; }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    char *y = malloc((size_t)n + 1);
    if (!y || fread(y, 1, (size_t)n, f) != (size_t)n) { perror(path); fclose(f); free(y); return NULL; }
    fclose(f);
    y[n] = 0;
    *len = (size_t)n;
    return y;
}

int main(int argc, char **argv)
{
    snaphash_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.device = -1; /* the current device */
    int32_t devs[64];
    int show_stats = 0, a = 1;
    for (; a < argc && argv[a][0] == '-' && argv[a][1]; a++) {
        if (!strcmp(argv[a], "-s")) show_stats = 1;
        else if (!strcmp(argv[a], "-g")) cfg.flags |= SNAPHASH_FLAG_GPU_ONLY;
        else if (!strcmp(argv[a], "-b")) cfg.flags |= SNAPHASH_FLAG_SPLIT_BLOCKS;
        else if (!strcmp(argv[a], "-z") && a + 1 < argc) cfg.deflate_depth = (uint32_t)strtoul(argv[++a], NULL, 10);
        else if (!strcmp(argv[a], "-t") && a + 1 < argc) cfg.host_threads = (uint32_t)strtoul(argv[++a], NULL, 10);
        else if (!strcmp(argv[a], "-d") && a + 1 < argc) {
            char *p = argv[++a];
            while (*p && cfg.n_devices < 64) {
                devs[cfg.n_devices++] = (int32_t)strtol(p, &p, 10);
                if (*p == ',') p++;
                else if (*p) return usage();
            }
            cfg.devices = devs;
        } else return usage();
    }
    argc -= a - 1;
    argv += a - 1;
    if (argc < 3) return usage();
    /* unxz / unpack-xz -F, in front of their names: the _ex entries with SNAPHASH_UNXZ_BCJ */
    snaphash_unxz_options uo;
    memset(&uo, 0, sizeof uo);
    if ((!strcmp(argv[1], "unxz") || !strcmp(argv[1], "unpack-xz")) && (!strcmp(argv[2], "-F") || !strcmp(argv[2], "-A"))) {
        uo.struct_size = sizeof uo;
        uo.flags = !strcmp(argv[2], "-A") ? SNAPHASH_UNXZ_CHAINS : SNAPHASH_UNXZ_BCJ; /* -A: any chain liblzma reads */
        for (int i = 2; i + 1 < argc; i++) argv[i] = argv[i + 1];
        argc--;
        if (argc < 3) return usage();
    }
    if (!strcmp(argv[1], "plan")) { /* what the planner would do with these files: no device is touched */
        size_t n = (size_t)argc - 2;
        uint64_t *lens = malloc(n * sizeof *lens);
        uint8_t *on_host = malloc(n);
        for (size_t i = 0; i < n; i++) {
            struct stat st;
            if (stat(argv[2 + i], &st) != 0) { perror(argv[2 + i]); return 2; }
            lens[i] = (uint64_t)st.st_size;
        }
        snaphash_plan_model pm;
        memset(&pm, 0, sizeof pm);
        pm.struct_size = sizeof pm;
        pm.n_devices = cfg.n_devices ? cfg.n_devices : 1;
        pm.host_threads = cfg.host_threads;
        pm.from_files = 1;
#if defined(__x86_64__)
        __builtin_cpu_init(); /* as a ctx would plan: where a host thread can run eight streams side by side, it counts on it */
        if (__builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw")) pm.host_lane_gain_pct = 240;
#endif
        int prc = snaphash_plan_streams(lens, n, &pm, on_host);
        if (prc) { fprintf(stderr, "snaphash: plan: %s\n", snaphash_strerror(prc)); return 1; }
        for (size_t i = 0; i < n; i++) printf("%s  %s\n", on_host[i] ? "host" : "gpu ", argv[2 + i]);
        fprintf(stderr, "snaphash: plan for %u usable CPUs: %llu streams / %llu B on %u host thread(s), modelled %.3f ms; GPU part modelled %.3f ms\n",
                snaphash_usable_cpus(), (unsigned long long)pm.host_streams, (unsigned long long)pm.host_bytes, pm.host_threads_used,
                pm.host_seconds * 1e3, pm.gpu_seconds * 1e3);
        free(lens); free(on_host);
        return 0;
    }
    snaphash_ctx *c = NULL;
    /* no engine option given: NULL config, so that SNAPHASH_DEVICES / SNAPHASH_HOST_THREADS apply (snaphash.h) */
    int rc = snaphash_init((cfg.n_devices || cfg.host_threads || cfg.flags || cfg.deflate_depth) ? &cfg : NULL, &c);
    if (rc) return die(NULL, rc, "snaphash_init");
    int ret = 0;
    if (!strcmp(argv[1], "hash")) {
        size_t n = (size_t)argc - 2;
        uint8_t *d = malloc(64 * n);
        rc = snaphash_sha512_files(c, (const char *const *)(argv + 2), n, d, NULL);
        if (rc) ret = die(c, rc, "hash");
        for (size_t i = 0; !rc && i < n; i++) {
            for (int b = 0; b < 64; b++) printf("%02x", d[64 * i + b]);
            printf("  %s\n", argv[2 + i]);
        }
        free(d);
    } else if (!strcmp(argv[1], "tree") && argc == 4) {
        char *y = NULL;
        size_t len = 0;
        rc = snaphash_tree(c, argv[2], argv[3], &y, &len);
        if (rc) ret = die(c, rc, "tree");
        else fwrite(y, 1, len, stdout);
        snaphash_free(y);
    } else if (!strcmp(argv[1], "write") && argc == 4) {
        rc = snaphash_write_hashes(c, argv[2], argv[3]);
        if (rc) ret = die(c, rc, "write");
    } else if (!strcmp(argv[1], "verify") && (argc == 4 || argc == 5)) {
        size_t len = 0;
        char *y = slurp(argv[3], &len);
        if (!y) { snaphash_destroy(c); return 2; }
        snaphash_mismatch m;
        rc = snaphash_verify(c, argv[2], argc == 5 ? argv[4] : NULL, y, len, &m);
        if (rc) ret = die(c, rc, "verify");
        else printf("OK\n");
        free(y);
    } else if (!strcmp(argv[1], "build") && argc != 4) {
        ret = usage();
    } else if (!strcmp(argv[1], "build") || !strcmp(argv[1], "build-xz") || !strcmp(argv[1], "build-bz2")) {
        const int xz = !strcmp(argv[1], "build-xz"), bz2 = !strcmp(argv[1], "build-bz2");
        /* build-xz's own options, in front of its two names: any of them goes through snaphash_tar_create_xz_ex */
        snaphash_xz_options xo;
        memset(&xo, 0, sizeof xo);
        xo.struct_size = sizeof xo;
        xo.check = 4;
        int xz_ex = 0, bad = 0;
        const char *cmd = argv[1];
        while (xz && argc > 4 && !bad) {
            int id = -1;
            if (!strcmp(argv[2], "-c")) { xo.flags |= SNAPHASH_XZ_SELF_CHECK; argv++; argc--; }
            else if (!strcmp(argv[2], "-B") && argc > 5) {
                xo.block_size = (uint64_t)strtoull(argv[3], NULL, 10) * 1024u;
                if (xo.block_size == 0) bad = 1;
                argv += 2; argc -= 2;
            } else if (!strcmp(argv[2], "-C") && argc > 5 && (id = xz_check_id(argv[3])) >= 0) { xo.check = (uint32_t)id; argv += 2; argc -= 2; }
            else if (!strcmp(argv[2], "-F") && argc > 5 && xz_filter_arg(argv[3], &xo)) { argv += 2; argc -= 2; }
            else if (!strcmp(argv[2], "-L") && argc > 5 && xz_level(argv[3]) >= 0) { xo.level = (uint32_t)xz_level(argv[3]); argv += 2; argc -= 2; }
            else bad = 1;
            xz_ex = 1;
        }
        /* build-bz2's, the same way: any of them goes through snaphash_tar_create_bz2_ex */
        snaphash_bz2_options bo;
        memset(&bo, 0, sizeof bo);
        bo.struct_size = sizeof bo;
        int bz2_ex = 0;
        while (bz2 && argc > 4 && !bad) {
            if (!strcmp(argv[2], "-c")) { bo.flags |= SNAPHASH_BZ2_SELF_CHECK; argv++; argc--; }
            else if (!strcmp(argv[2], "-L") && argc > 5 && (bo.level = bz2_level(argv[3])) != 0) { argv += 2; argc -= 2; }
            else bad = 1;
            bz2_ex = 1;
        }
        if (bad || argc != 4) { snaphash_destroy(c); return usage(); }
        /* the exclude rule is writeHashes' own: every path that starts with <dir>/DEBIAN (build.go:229) */
        size_t dl = strlen(argv[2]);
        while (dl > 1 && argv[2][dl - 1] == '/') dl--;
        char *dir = malloc(dl + 1), *excl = malloc(dl + 8), *ypath = malloc(dl + 32);
        memcpy(dir, argv[2], dl);
        dir[dl] = 0;
        sprintf(excl, "%s/DEBIAN", dir);
        sprintf(ypath, "%s/DEBIAN/hashes.yaml", dir);
        char *y = NULL;
        size_t len = 0;
        uint8_t dig[64];
        rc = xz_ex ? snaphash_tar_create_xz_ex(c, argv[3], dir, excl, &xo, &y, &len, dig)
             : xz  ? snaphash_tar_create_xz(c, argv[3], dir, excl, &y, &len, dig)
             : bz2_ex ? snaphash_tar_create_bz2_ex(c, argv[3], dir, excl, &bo, &y, &len, dig)
             : bz2 ? snaphash_tar_create_bz2(c, argv[3], dir, excl, &y, &len, dig)
                   : snaphash_tar_create(c, argv[3], dir, excl, &y, &len, dig);
        if (rc) ret = die(c, rc, cmd);
        else {
            if (show_stats && (xo.flags & SNAPHASH_XZ_SELF_CHECK)) print_xz_selfcheck(c, cmd);
            if (show_stats && (xo.filter || xo.chain_len)) print_xz_filter(c, cmd);
            if (show_stats && (bo.flags & SNAPHASH_BZ2_SELF_CHECK)) print_bz2_selfcheck(c, cmd);
            (void)mkdir(excl, 0755); /* os.MkdirAll(debianDir, 0755), error ignored (build.go:218-219) */
            FILE *f = fopen(ypath, "wb");
            if (!f || fwrite(y, 1, len, f) != len || fclose(f)) { perror(ypath); ret = 2; }
            for (int b = 0; !ret && b < 64; b++) printf("%02x", dig[b]);
            if (!ret) printf("  %s\n", argv[3]);
        }
        snaphash_free(y);
        free(dir); free(excl); free(ypath);
    } else if (!strcmp(argv[1], "gzip") && argc == 4) {
        size_t len = 0, zl = 0;
        char *in = slurp(argv[2], &len);
        if (!in) { snaphash_destroy(c); return 2; }
        void *z = NULL;
        rc = snaphash_gzip_buffer(c, in, len, &z, &zl);
        if (rc) ret = die(c, rc, "gzip");
        else {
            FILE *f = fopen(argv[3], "wb");
            if (!f || fwrite(z, 1, zl, f) != zl || fclose(f)) { perror(argv[3]); ret = 2; }
        }
        snaphash_free(z);
        free(in);
    } else if (!strcmp(argv[1], "bzip2") && argc >= 4) {
        size_t len = 0, zl = 0;
        unsigned level = 9;
        int self = 0, at = 2;
        while (argc - at > 2) { /* the options, in front of the two names */
            if (!strcmp(argv[at], "-c")) { self = 1; at += 1; }
            else if (!strcmp(argv[at], "-L") && argc - at > 3 && (level = bz2_level(argv[at + 1])) != 0) at += 2;
            else { snaphash_destroy(c); return usage(); }
        }
        if (argc - at != 2) { snaphash_destroy(c); return usage(); }
        snaphash_bz2_options bo;
        memset(&bo, 0, sizeof bo);
        bo.struct_size = sizeof bo;
        bo.flags = SNAPHASH_BZ2_SELF_CHECK;
        bo.level = level;
        char *in = slurp(argv[at], &len);
        if (!in) { snaphash_destroy(c); return 2; }
        void *z = NULL;
        rc = self ? snaphash_bzip2_buffer_ex(c, in, len, &bo, &z, &zl) : snaphash_bzip2_buffer(c, in, len, (uint32_t)level, &z, &zl);
        if (rc) ret = die(c, rc, "bzip2");
        else {
            if (show_stats && self) print_bz2_selfcheck(c, "bzip2");
            FILE *f = fopen(argv[at + 1], "wb");
            if (!f || fwrite(z, 1, zl, f) != zl || fclose(f)) { perror(argv[at + 1]); ret = 2; }
        }
        snaphash_free(z);
        free(in);
    } else if (!strcmp(argv[1], "xz") && argc >= 4) {
        size_t len = 0, zl = 0;
        uint64_t block = 0;
        int have_block = 0, check = -1, self = 0; /* -1: no -C, the entry point that takes no Check */
        uint32_t level = 0;
        snaphash_xz_options xo;
        memset(&xo, 0, sizeof xo);
        for (int i = 4; i < argc;) {
            if (!strcmp(argv[i], "-c")) { self = 1; i += 1; continue; }
            if (i + 1 >= argc) { snaphash_destroy(c); return usage(); }
            if (!strcmp(argv[i], "-B")) {
                block = (uint64_t)strtoull(argv[i + 1], NULL, 10) * 1024u;
                have_block = 1;
            } else if (!strcmp(argv[i], "-C") && xz_check_id(argv[i + 1]) >= 0) check = xz_check_id(argv[i + 1]);
            else if (!strcmp(argv[i], "-F") && xz_filter_arg(argv[i + 1], &xo)) ;
            else if (!strcmp(argv[i], "-L") && xz_level(argv[i + 1]) >= 0) level = (uint32_t)xz_level(argv[i + 1]);
            else { snaphash_destroy(c); return usage(); }
            i += 2;
        }
        const int filter = xo.filter || xo.chain_len;
        xo.struct_size = sizeof xo;
        xo.flags = self ? SNAPHASH_XZ_SELF_CHECK : 0;
        xo.block_size = block;
        xo.check = check < 0 ? 4u : (uint32_t)check;
        xo.level = level;
        char *in = slurp(argv[2], &len);
        if (!in) { snaphash_destroy(c); return 2; }
        void *z = NULL;
        rc = (have_block && block == 0) ? SNAPHASH_EINVAL
             : self || filter || level  ? snaphash_xz_buffer_ex(c, in, len, &xo, &z, &zl)
             : check < 0                ? snaphash_xz_buffer(c, in, len, block, &z, &zl)
                                        : snaphash_xz_buffer_check(c, in, len, block, (uint32_t)check, &z, &zl);
        if (rc) ret = die(c, rc, "xz");
        else {
            if (show_stats && self) print_xz_selfcheck(c, "xz");
            if (show_stats && filter) print_xz_filter(c, "xz");
            FILE *f = fopen(argv[3], "wb");
            if (!f || fwrite(z, 1, zl, f) != zl || fclose(f)) { perror(argv[3]); ret = 2; }
        }
        snaphash_free(z);
        free(in);
    } else if ((!strcmp(argv[1], "gunzip") || !strcmp(argv[1], "bunzip2") || !strcmp(argv[1], "unxz")) && argc == 4) {
        const int xz = !strcmp(argv[1], "unxz");
        const int bz = xz || !strcmp(argv[1], "bunzip2");
        size_t len = 0, ol = 0;
        char *in = slurp(argv[2], &len);
        if (!in) { snaphash_destroy(c); return 2; }
        void *o = NULL;
        rc = xz && uo.flags ? snaphash_unxz_buffer_ex(c, in, len, &uo, &o, &ol) : xz ? snaphash_unxz_buffer(c, in, len, &o, &ol) : bz ? snaphash_bunzip2_buffer(c, in, len, &o, &ol) : snaphash_gunzip_buffer(c, in, len, &o, &ol);
        if (rc) ret = die(c, rc, argv[1]);
        else {
            FILE *f = fopen(argv[3], "wb");
            if (!f || fwrite(o, 1, ol, f) != ol || fclose(f)) { perror(argv[3]); ret = 2; }
        }
        if (show_stats && !bz && (cfg.flags & SNAPHASH_FLAG_SPLIT_BLOCKS)) print_block_stats(c, argv[1]);
        if (show_stats && xz && uo.flags && !rc) print_xz_filter(c, argv[1]);
        snaphash_free(o);
        free(in);
    } else if ((!strcmp(argv[1], "unpack") || !strcmp(argv[1], "unpack-bz2") || !strcmp(argv[1], "unpack-xz")) && (argc == 4 || argc == 5)) {
        const int xz = !strcmp(argv[1], "unpack-xz");
        const int bz = xz || !strcmp(argv[1], "unpack-bz2");
        size_t len = 0;
        char *y = NULL;
        if (argc == 5 && !(y = slurp(argv[4], &len))) { snaphash_destroy(c); return 2; }
        snaphash_mismatch m;
        uint8_t dig[64];
        rc = xz && uo.flags ? snaphash_tar_unpack_xz_ex(c, argv[2], argv[3], y, len, &uo, &m, dig)
             : xz ? snaphash_tar_unpack_xz(c, argv[2], argv[3], y, len, &m, dig)
             : bz ? snaphash_tar_unpack_bz2(c, argv[2], argv[3], y, len, &m, dig)
                  : snaphash_tar_unpack(c, argv[2], argv[3], y, len, &m, dig);
        if (rc) ret = die(c, rc, argv[1]);
        else printf("OK\n");
        if (show_stats) {
            snaphash_unpack_stats us;
            us.struct_size = sizeof us;
            if (!snaphash_get_unpack_stats(c, &us))
                fprintf(stderr, "%s: %llu %s bytes -> %llu tar bytes, %llu members, %llu %s (%llu on the GPU), %llu bytes decoded on "
                                "the host, %s kernels %.2f ms, wall %.2f ms\n",
                        argv[1], (unsigned long long)us.gz_bytes, xz ? "xz" : bz ? "bz2" : "gz", (unsigned long long)us.tar_bytes, (unsigned long long)us.members,
                        (unsigned long long)us.segments, bz ? "blocks" : "segments", (unsigned long long)us.gpu_segments,
                        (unsigned long long)us.host_bytes, xz ? "lzma2" : bz ? "bzip2" : "inflate", us.inflate_ms, us.wall_ms);
            if (!bz && (cfg.flags & SNAPHASH_FLAG_SPLIT_BLOCKS)) print_block_stats(c, argv[1]);
        }
        free(y);
    } else if (!strcmp(argv[1], "snap") && argc >= 4 && !strcmp(argv[2], "build")) {
        /* the options in front of the two names; -L -F -C -B go to the producer -Z names, and the library refuses what is not its */
        snaphash_snap_build_options opt;
        snaphash_xz_options xo;
        snaphash_bz2_options bo;
        memset(&opt, 0, sizeof opt);
        memset(&xo, 0, sizeof xo);
        memset(&bo, 0, sizeof bo);
        opt.struct_size = sizeof opt;
        opt.mtime = -1;
        xo.struct_size = sizeof xo;
        xo.check = 4;
        bo.struct_size = sizeof bo;
        int bad = 0, xz_opts = 0;
        const char *level = NULL;
        while (argc > 5 && !bad) {
            int id = -1;
            if (!strcmp(argv[3], "-c")) { opt.flags |= SNAPHASH_BUILD_CHECK; argv++; argc--; continue; }
            if (argc < 7) { bad = 1; break; }
            if (!strcmp(argv[3], "-Z")) {
                opt.data_codec = !strcmp(argv[4], "gz") ? SNAPHASH_DATA_GZ : !strcmp(argv[4], "bz2") ? SNAPHASH_DATA_BZ2 : !strcmp(argv[4], "xz") ? SNAPHASH_DATA_XZ : 99u;
                bad = opt.data_codec == 99u;
            } else if (!strcmp(argv[3], "-L")) level = argv[4];
            else if (!strcmp(argv[3], "-B")) { xo.block_size = (uint64_t)strtoull(argv[4], NULL, 10) * 1024u; bad = xo.block_size == 0; xz_opts = 1; }
            else if (!strcmp(argv[3], "-C") && (id = xz_check_id(argv[4])) >= 0) { xo.check = (uint32_t)id; xz_opts = 1; }
            else if (!strcmp(argv[3], "-F") && xz_filter_arg(argv[4], &xo)) xz_opts = 1;
            else bad = 1;
            argv += 2; argc -= 2;
        }
        if (level && opt.data_codec == SNAPHASH_DATA_BZ2) { bo.level = bz2_level(level); bad |= bo.level == 0; opt.bz2 = &bo; }
        else if (level) { bad |= xz_level(level) < 0; xo.level = (uint32_t)(xz_level(level) > 0); xz_opts = 1; }
        if (xz_opts) opt.xz = &xo; /* (with another codec: the library's refusal) */
        if (bad || argc != 5) ret = usage();
        else {
            snaphash_snap_build_stats bs;
            uint8_t adig[64], sdig[64];
            bs.struct_size = sizeof bs;
            rc = snaphash_snap_build(c, argv[argc - 2], argv[argc - 1], &opt, adig, sdig, &bs);
            if (rc) ret = die(c, rc, "snap build");
            else {
                const char *member = opt.data_codec == SNAPHASH_DATA_XZ ? "data.tar.xz" : opt.data_codec == SNAPHASH_DATA_BZ2 ? "data.tar.bz2" : "data.tar.gz";
                for (int i = 0; i < 64; i++) printf("%02x", sdig[i]);
                printf("  %s\n", argv[argc - 1]);
                if (show_stats)
                    fprintf(stderr, "snap build: %llu bytes (%s %llu of %llu tar bytes, %llu members; control.tar.gz %llu); data %.1f ms, control %.1f ms, "
                                    "container %.1f ms, wall %.1f ms; self-check: %llu chunks, %.3f ms\n",
                            (unsigned long long)bs.snap_bytes, member, (unsigned long long)bs.data_bytes, (unsigned long long)bs.tar_bytes, (unsigned long long)bs.members,
                            (unsigned long long)bs.control_bytes, bs.data_ms, bs.control_ms, bs.ar_ms, bs.wall_ms, (unsigned long long)bs.check_chunks, bs.check_ms);
                if (show_stats && opt.data_codec == SNAPHASH_DATA_XZ && (xo.filter || xo.chain_len)) print_xz_filter(c, "snap build");
            }
        }
    } else if (!strcmp(argv[1], "snap") && argc >= 4) {
        /* -x in front of the verb: the session routes .xz members to the .xz engine */
        snaphash_snap_open_options so = {sizeof so, 0};
        if (!strcmp(argv[2], "-x")) { so.flags = SNAPHASH_SNAP_XZ; argv++; argc--; }
        if (so.flags && argc >= 4 && !strcmp(argv[2], "-A")) { so.flags |= SNAPHASH_SNAP_XZ_CHAINS; argv++; argc--; } /* -x -A: any chain */
        const char *verb = argv[2], *file = argv[argc - 1];
        const int takes_arg = !strcmp(verb, "cat-control") || !strcmp(verb, "cat-meta") || !strcmp(verb, "unpack");
        const int known = takes_arg || !strcmp(verb, "ls") || !strcmp(verb, "audit");
        snaphash_snap *sn = NULL;
        if (!known || argc != (takes_arg ? 5 : 4)) ret = usage();
        else if ((rc = snaphash_snap_open_ex(c, file, &so, &sn)) != 0) ret = die(c, rc, "snap");
        else if (!strcmp(verb, "ls")) {
            for (size_t i = 0; i < snaphash_snap_members(sn); i++) {
                const char *nm;
                uint64_t off, sz;
                snaphash_snap_member_info(sn, i, &nm, &off, &sz);
                printf("%10llu %10llu %s\n", (unsigned long long)sz, (unsigned long long)off, nm);
            }
        } else if (!strcmp(verb, "cat-control") || !strcmp(verb, "cat-meta")) {
            void *p = NULL;
            size_t len = 0;
            rc = verb[4] == 'c' ? snaphash_snap_control_member(sn, argv[3], &p, &len) : snaphash_snap_meta_member(sn, argv[3], &p, &len);
            if (rc) ret = die(c, rc, verb);
            else if (!p) { fprintf(stderr, "snaphash: %s: no member %s\n", verb, argv[3]); ret = 1; }
            else fwrite(p, 1, len, stdout);
            snaphash_free(p);
        } else {
            snaphash_mismatch m;
            uint8_t dig[64];
            rc = !strcmp(verb, "audit") ? snaphash_snap_audit(sn, &m, dig) : snaphash_snap_unpack(sn, argv[3], 1, &m, dig);
            if (rc) ret = die(c, rc, verb);
            else printf("OK\n");
            if (show_stats) {
                snaphash_unpack_stats us;
                snaphash_snap_stats ss;
                us.struct_size = sizeof us;
                ss.struct_size = sizeof ss;
                if (!snaphash_get_unpack_stats(c, &us))
                    fprintf(stderr, "snap %s: %llu compressed bytes -> %llu tar bytes, %llu members, %llu segments (%llu on the GPU), "
                                    "%llu bytes decoded on the host, decode kernels %.2f ms, wall %.2f ms\n",
                            verb, (unsigned long long)us.gz_bytes, (unsigned long long)us.tar_bytes, (unsigned long long)us.members,
                            (unsigned long long)us.segments, (unsigned long long)us.gpu_segments, (unsigned long long)us.host_bytes,
                            us.inflate_ms, us.wall_ms);
                if (!snaphash_snap_get_stats(sn, &ss))
                    fprintf(stderr, "snap %s: data.tar decoded %llu time(s), control.tar %llu; CRCs: %llu on the device (%.3f ms), %llu on host threads\n",
                            verb, (unsigned long long)ss.data_decodes, (unsigned long long)ss.control_decodes,
                            (unsigned long long)ss.device_crc_ranges, ss.device_crc_ms, (unsigned long long)ss.host_crc_ranges);
            }
        }
        snaphash_snap_close(sn);
    } else if (!strcmp(argv[1], "cmp") && argc >= 4 && argc % 2 == 0) {
        size_t n = ((size_t)argc - 2) / 2;
        const char **pa = malloc(n * sizeof *pa), **pb = malloc(n * sizeof *pb);
        uint8_t *eq = malloc(n);
        for (size_t i = 0; i < n; i++) { pa[i] = argv[2 + 2 * i]; pb[i] = argv[3 + 2 * i]; }
        rc = snaphash_files_equal(c, pa, pb, n, eq);
        if (rc) ret = die(c, rc, "cmp");
        for (size_t i = 0; !rc && i < n; i++) {
            printf("%s %s %s\n", eq[i] ? "equal " : "differ", pa[i], pb[i]);
            if (!eq[i]) ret = 1;
        }
        free(pa); free(pb); free(eq);
    } else if (!strcmp(argv[1], "dirupdated") && (argc == 4 || argc == 5)) {
        char *names = NULL;
        size_t count = 0;
        rc = snaphash_dir_updated(c, argv[2], argv[3], argc == 5 ? argv[4] : "", &names, &count);
        if (rc) ret = die(c, rc, "dirupdated");
        const char *p = names;
        for (size_t i = 0; !rc && i < count; i++, p += strlen(p) + 1) printf("%s\n", p);
        snaphash_free(names);
    } else {
        ret = usage();
    }
    if (show_stats && ret != 2) {
        snaphash_stats st;
        snaphash_stats_ex ex;
        memset(&ex, 0, sizeof ex);
        ex.struct_size = sizeof ex;
        snaphash_targz_stats tz;
        snaphash_get_stats(c, &st);
        snaphash_get_stats_ex(c, &ex);
        snaphash_get_targz_stats(c, &tz);
        fprintf(stderr, "snaphash: %llu B in %llu streams, kernels %.2f ms, h2d %.2f ms; host threads hashed %llu B\n",
                (unsigned long long)st.bytes_hashed, (unsigned long long)st.streams, st.kernel_ms, st.h2d_ms,
                (unsigned long long)ex.host_bytes);
        if (tz.tar_bytes)
            fprintf(stderr, "snaphash: tar %llu B -> %llu B written, %llu members, %llu chunks (%llu stored), compressor kernels %.2f ms, wall %.1f ms\n",
                    (unsigned long long)tz.tar_bytes, (unsigned long long)tz.gz_bytes, (unsigned long long)tz.members,
                    (unsigned long long)tz.chunks, (unsigned long long)tz.stored_chunks, tz.deflate_ms, tz.wall_ms);
    }
    snaphash_destroy(c);
    return ret;
}
