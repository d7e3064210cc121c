"""The GPU inflate path at its own edges (inflate_kernels.hip: flush scan, block scan, decode, hole fill, concat; their
driver in unpack.inc): the streams of tests/inflate_edge_streams.py through Context.gunzip_buffer in both configurations
(conftest.py snaphash_mode), flush mode and -- FLAG_SPLIT_BLOCKS -- block mode.  zlib is the reference for every byte;
tests/test_inflate_edges_host.py shows on the CPU that each stream has the shape it claims and that inflate_core.h
decodes it, so a failure here points at the kernels or the driver.  Statistics that follow from the linking rule are
computed from the builders' facts (inflate_edge_streams.plan_flush), never from a run of the library."""
import io
import tarfile
import zlib

import pytest

import inflate_edge_streams as E
from snappy_amd import Context, _lib, getHashes
from test_gpu_inflate_blocks import bh, split_ctx, tree  # noqa: F401  (bh: a fixture)
from test_gpu_unpack import umask_022  # noqa: F401  (a fixture)
from test_inflate_blocks_host import blocks, scan

pytestmark = pytest.mark.gpu

HOST_PIECE = 8 << 20  # unpack.inc kHostPiece: the default configuration's pieces


def check(c, r, mode, piece=HOST_PIECE):
    """gunzip_buffer gives zlib's bytes, and who decoded what is what the linking rule says."""
    want = zlib.decompress(r["gz"], 31)
    assert want == r["data"]
    assert c.gunzip_buffer(r["gz"]) == want
    st = c.unpack_stats()
    assert st["tar_bytes"] == len(want) and st["gz_bytes"] == len(r["gz"]), st
    linked, host = E.plan_flush(r["gz"][10:], r["starts"], r["lens"], piece if mode == "gpu_only" else HOST_PIECE)
    assert st["host_bytes"] == host and st["segments"] == len(r["lens"]), (st, linked, host)
    assert st["gpu_segments"] == (linked if mode == "gpu_only" else 0), (st, linked)
    return st


def refused_then_good(c, bad, good):
    with pytest.raises(_lib.SnaphashError) as e:
        c.gunzip_buffer(bad)
    assert e.value.code == _lib.EFORMAT
    assert c.gunzip_buffer(good["gz"]) == good["data"]


def test_item1_far_holes_of_holes(snaphash_mode):
    """inflate_fill_kernel and gpu_fill_concat's ordered sweep: segments in which every symbol is a hole at distance
    32 768 (the top of the uint16 slot's range), each hole's byte some 42 segments back and a hole itself."""
    r = E.far_hole_chain()
    with Context(device=0) as c:
        st = check(c, r, snaphash_mode)
        assert st["host_bytes"] == 0
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == st["segments"] == 132


def test_item2_holes_across_tiny_and_empty_segments(snaphash_mode):
    """inflate_fill_kernel's segment lookup (the walk back over links whose off lies past the byte): holes whose bytes
    lie several segments back, across segments of 0, 1, 2 and 3 bytes."""
    r = E.tiny_segments()
    with Context(device=0) as c:
        st = check(c, r, snaphash_mode)
        assert st["host_bytes"] == 0
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == st["segments"] == len(r["lens"])


@pytest.mark.parametrize("first", [50000, 20000])
def test_item3_window_in_front_of_a_piece(snaphash_mode, first):
    """d_win and wlen = min(32768, o0 - m0) in gpu_fill_concat: pieces of 64 KiB, the second one's first match exactly
    wlen back from its first byte (wlen 32 768, and 20 000: all the member has produced); one byte further is in front
    of the member and must be EFORMAT."""
    r = E.window_edge(first)
    with Context(device=0, staging_bytes=E.PIECE_FLOOR) as c:
        st = check(c, r, snaphash_mode, E.PIECE_FLOOR)
        assert st["host_bytes"] == 0
        if first < E.WINDOW:
            refused_then_good(c, E.window_edge(first, 1)["gz"], r)
    with Context(device=0) as c:  # one piece: the same bytes without a window
        check(c, r, snaphash_mode)


@pytest.mark.parametrize("lead, pad", [(0, 0), (10, 0), (0, 1100 << 10)])
def test_item3_reference_in_front_of_a_later_member(snaphash_mode, lead, pad):
    """The fill kernel's g < 0 guard with wlen = 0 at a member's start (and fill_holes_host's `avail`): a second member
    reaching in front of its own start, where the first member's bytes lie in the output.  zlib: "invalid distance too
    far back"; here EFORMAT in flush and block mode, never the other member's bytes, and the context goes on working."""
    r = E.reach_before_member(lead, pad)
    with pytest.raises(zlib.error, match="too far back"):
        zlib.decompress(r["gz"][len(r["good"]["gz"]):], 31)
    with Context(device=0) as c:
        refused_then_good(c, r["gz"], r["good"])
    with split_ctx() as c:
        refused_then_good(c, r["gz"], r["good"])
        if pad:
            assert c.gunzip_buffer(r["good"]["gz"] * 2) == r["good"]["data"] * 2


def test_item4_more_false_candidates_than_the_scan_keeps(snaphash_mode):
    """inflate_scan_kernel past cand_cap and the cut of the candidates to the launch's slots: two candidates per four
    bytes.  Which candidates survive is arbitrary (the scan appends them unordered), so only the bytes and the byte
    counts are asserted; that the call returns at all says every piece advanced."""
    r = E.dense_false_candidates()
    want = zlib.decompress(r["gz"], 31)
    for make in (lambda: Context(device=0), lambda: Context(device=0, staging_bytes=E.PIECE_FLOOR), split_ctx):
        with make() as c:
            assert c.gunzip_buffer(r["gz"]) == want == r["data"]
            st = c.unpack_stats()
            assert st["tar_bytes"] == len(want) and st["gz_bytes"] == len(r["gz"]), st


@pytest.mark.parametrize("kind", sorted(E.SLOT_PATTERNS))
def test_item5_segments_at_the_slot_capacity(snaphash_mode, kind):
    """kInflateSlotSyms, kInfOverflow and nl == 0 -> host_run: segments of exactly 69 632 symbols are the slots', of
    69 633 the host decoder's, and chains and host stretches follow each other inside one member."""
    r = E.slot_capacity(kind)
    with Context(device=0) as c:
        st = check(c, r, snaphash_mode)
        assert st["host_bytes"] == sum(n for n in r["lens"] if n > E.SLOT_SYMS)


@pytest.mark.parametrize("rle", [False, True])
def test_item5_block_longer_than_a_block_slot(snaphash_mode, bh, rle):
    """Block mode's kInflateBlockSlotSyms: a run that zlib packs into blocks of a megabyte and more is the host
    decoder's, the stored stretch in front of it the slots'."""
    r = E.long_block(rle)
    longer = [o for _, _, o in blocks(bh, r["raw"])[0] if o > E.BLOCK_SLOT_SYMS]
    assert longer
    with split_ctx() as c:
        assert c.gunzip_buffer(r["gz"]) == zlib.decompress(r["gz"], 31) == r["data"]
        st, bs = c.unpack_stats(), c.block_scan_stats()
        # the long blocks are the host's; the 16 whole stored blocks of 65 535 bytes in front of them end on candidates
        # and fit a slot, so the chain from the member's start links them
        assert bs["host_blocks"] >= 1 and sum(longer) <= st["host_bytes"] <= len(r["data"]) - 16 * 65535, (st, bs)
        assert st["segments"] > bs["host_blocks"] and bs["bits_scanned"] >= 8 * len(r["raw"]), (st, bs)


@pytest.mark.parametrize("kind", ["level0", "on_piece_end", "final_on_piece_end"])
def test_item6_pieces_that_end_inside_or_on_a_segment(snaphash_mode, kind):
    """kInfTruncated and `pos >= pn` in the link loop: pieces of 64 KiB against stored blocks of 65 540 bytes (no piece
    holds a whole segment: every one the host's), of exactly a piece, and with the final block's end on a piece's end."""
    r = E.piece_cuts(kind)
    with Context(device=0, staging_bytes=E.PIECE_FLOOR) as c:
        st = check(c, r, snaphash_mode, E.PIECE_FLOOR)
        if snaphash_mode == "gpu_only":
            assert (st["gpu_segments"], st["host_bytes"]) == {"level0": (1, 6 * 65535), "on_piece_end": (6, 0),
                                                              "final_on_piece_end": (4, 0)}[kind]


def test_item7_block_types_and_codes_the_corpora_never_have(snaphash_mode):
    """inflate_decode_kernel (inflate_run with its tables in LDS, on one lane): fixed-Huffman blocks, literal and
    distance codes of 15 bits, a single-symbol distance code, runs of 258-byte matches at distances 1, 15, 16, 17 and
    18 (the d >= 16 split of the copy loop), Z_HUFFMAN_ONLY and a window of 512, each cut by flush points into several
    segments that fit a slot."""
    with Context(device=0) as c:
        for name, r in E.decode_streams().items():
            st = check(c, r, snaphash_mode)
            assert st["host_bytes"] == 0, name
            if snaphash_mode == "gpu_only":
                assert st["gpu_segments"] == st["segments"] == len(r["lens"]), (name, st)


_scan_want = {}  # the CPU checker's counts, shared by the two configurations


def scan_case(c, bh, key, r):
    """One call: the bytes are zlib's, and the block scan counted what inf_dynamic_ok finds on the same pieces."""
    assert c.gunzip_buffer(r["gz"]) == r["data"], key
    if key not in _scan_want:
        _scan_want[key] = sum(len(scan(bh, r["gz"][a:a + n])) for a, n in r["pieces"])
    bs = c.block_scan_stats()
    assert bs["bits_scanned"] == 8 * sum(n for _, n in r["pieces"]), (key, bs)
    assert bs["candidates"] == _scan_want[key], (key, bs, _scan_want[key])
    assert bs["linked"] + bs["unreached"] == bs["candidates"], (key, bs)
    return bs


def test_item8_headers_moved_across_a_tile_edge(snaphash_mode, bh):
    """inflate_block_scan_kernel's tile load and `j < tbytes`: a shortest header starting on each of the last 16 bits
    of a tile and the first 16 of the next, one stream per position (only a count is visible: a lost or doubled offset
    shows at its position); the longest header (2233 bits) from a tile's last bits, which needs the whole halo."""
    with split_ctx() as c:
        for d in E.SCAN_EDGE_RANGE:
            assert scan_case(c, bh, ("edge", d), E.scan_edge(d))["candidates"] == 1
        for d in E.SCAN_HALO_RANGE:
            assert scan_case(c, bh, ("halo", d), E.scan_halo(d))["candidates"] == 1


def test_item8_header_at_the_piece_end(snaphash_mode, bh):
    """inf_dynamic_lengths' `at > n * 8` on the device and the tile's zero fill past the piece: a header that ends on
    the piece's last bit counts, one bit later it does not."""
    with split_ctx() as c:
        for kind in ("long", "min"):
            for d, found in ((-9, 1), (-1, 1), (0, 1), (1, 0), (8, 0)):
                assert scan_case(c, bh, ("end", kind, d), E.scan_piece_end(d, kind))["candidates"] == found


def test_item8_queue_flushes_and_candidate_overflow(snaphash_mode, bh):
    """The per-wave queue of inflate_block_scan_kernel (flush(64) with a remainder shifted down, several times a tile)
    and a count past bcand_cap: more candidates than are kept, all of them counted."""
    with split_ctx() as c:
        assert scan_case(c, bh, "dense", E.scan_dense())["candidates"] >= 600
        assert scan_case(c, bh, "overflow", E.scan_overflow())["candidates"] > E.SPLIT_MIN // 64 + 4096


@pytest.mark.parametrize("length", E.SCAN_TAILS)
def test_item8_second_piece_of_any_length(snaphash_mode, bh, length):
    """The byte-wise tail of the tile load: a last piece of 4096 k, 4096 k - 1, + 1 and + 3 bytes with headers on its
    last bits and at its last tile edge."""
    with split_ctx() as c:
        assert scan_case(c, bh, ("tail", length), E.scan_tail(length))["candidates"] == 4
        assert c.unpack_stats()["host_bytes"] == 0


def tar_of(files):
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as t:
        for name, data in files.items():
            ti = tarfile.TarInfo("./" + name)
            ti.size, ti.mode, ti.mtime = len(data), 0o644, 1500000000
            t.addfile(ti, io.BytesIO(data))
    return buf.getvalue()


def test_edge_streams_through_tar_unpack_with_verify(snaphash_mode, tmp_path, umask_022):
    """gpu_fill_concat with keep_dev and DecodedStream::reserve_dev: the decoded bytes stay in HBM for Verify while d_out grows and is
    copied, piece after piece with the window carried along (pieces of 64 KiB); the archives have the shapes of items
    5 (segments at and over the slot capacity) and 6 (stored blocks no piece holds) and plain short segments."""
    files = {"text": E.text(2500000, 50), "blob": E.noise(300000, 51), "zeros": bytes(100000), "empty": b"", "x/y": b"deep\n"}
    tar = tar_of(files)
    cycle = [E.SLOT_SYMS, E.SLOT_SYMS + 1, 20000, E.SLOT_SYMS]
    lens = (cycle * (len(tar) // sum(cycle) + 1))[:len(tar) // sum(cycle) * 4]
    lens.append(len(tar) - sum(lens))
    stored = E.Stream()
    for k in range(0, len(tar), 65535):
        stored.stored(tar[k:k + 65535])
    archives = {"slots": E.zlib_flushed(tar, lens)["gz"], "short": E.zlib_flushed(tar, [40000] * (len(tar) // 40000) + [len(tar) % 40000])["gz"],
                "stored": stored.result(stored.finish())["gz"]}
    yaml = None
    for name, gz in archives.items():
        assert zlib.decompress(gz, 31) == tar
        arc = str(tmp_path / (name + ".tar.gz"))
        with open(arc, "wb") as f:
            f.write(gz)
        for staging in (0, E.PIECE_FLOOR):
            with Context(device=0, staging_bytes=staging) as c:
                plain = str(tmp_path / ("%s_%d_plain" % (name, staging)))
                assert c.tar_unpack(arc, plain)[0] is None
                got = tree(plain)
                assert {k: got[k] for k in files} == files
                yaml = getHashes(plain, arc, c)
                assert c.tar_unpack(arc, str(tmp_path / ("%s_%d_verified" % (name, staging))), yaml)[0] is None
                st = c.unpack_stats()
                assert st["tar_bytes"] == len(tar) and st["members"] == len(files), st
                if name == "short":
                    assert st["host_bytes"] == 0, st
    # the Verify above read the decoded bytes: a digest that is off by one digit is found
    lines = yaml.split(b"\n")
    k = next(j for j in range(lines.index(b"- name: text"), len(lines)) if lines[j].startswith(b"  sha512: "))
    lines[k] = lines[k][:-1] + (b"0" if lines[k][-1:] != b"0" else b"1")
    with Context(device=0, staging_bytes=E.PIECE_FLOOR) as c:
        assert c.tar_unpack(arc, str(tmp_path / "tampered"), b"\n".join(lines))[0] is not None
