"""deflate_chunks_kernel (snappy_amd/csrc/deflate_kernels.hip) at its own edges.

The code construction: huff_lengths_wave and huff_codes_wave -- a rank count for the serial routine's radix sort, queue
heads in registers, a depth walk that is cut off, a ballot that sends the whole wave round again, five symbols a lane --
through snaphash_deflate_codes_device on the tables of tests/deflate_code_tables.py, a wave a table, one launch an
alphabet: the lengths, the codes and the number of trees built must equal the serial routines' (which
tests/test_deflate_codes_host.py holds against an independent reference), and no byte around the three result arrays may
change.  Most of those tables need a second tree or more; whole inputs practically never do.

The whole compressor: the inputs of tests/deflate_edge_inputs.py (sizes around the 1920-position segment, the 28800-byte
window and the chunk; a repeat at exactly the window's edge, from the previous chunk, in a chunk without a window; matches
of 257 to 259 bytes; the code length code's limiter; search depths 1 -- which the library raises to 4 -- and 128) through Context.gzip_buffer with staging
pieces of one and of three chunks: gzip must read them back and the bytes must equal the CPU model's
(tests/test_f3_host.py shows by the model's counters that every input has the shape it is named for)."""
import ctypes
import gzip

import numpy as np
import pytest

import deflate_code_tables as T
import deflate_edge_inputs as E
from test_deflate_codes_host import serial_tables
from test_f3_host import f3  # noqa: F401  (the CPU model and the serial code construction)

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("the DEFLATE kernel and its code construction: nothing in them is planned")]

CANARY = 256  # bytes on both sides of every result array


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def codes_ctx(built_lib):
    from snappy_amd import Context, _lib
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


def device_tables(c, n, max_bits, freq):
    """freq: uint32 [tables, n] -> (lens, codes, rounds) from the kernel's routines; asserts the canaries around them."""
    torch = _torch()
    nt = freq.shape[0]
    d_freq = torch.from_numpy(np.ascontiguousarray(freq, dtype=np.uint32).view(np.int32)).cuda()
    outs = []
    for nbytes in (nt * n, 4 * nt * n, 4 * nt):
        outs.append(torch.full((CANARY + nbytes + CANARY,), 0xA5, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    c.deflate_codes_device(d_freq.data_ptr(), nt, n, max_bits, *(o.data_ptr() + CANARY for o in outs))
    host = [o.cpu().numpy() for o in outs]
    for h in host:
        assert (h[:CANARY] == 0xA5).all() and (h[-CANARY:] == 0xA5).all(), "a byte outside the result arrays was written"
    lens = host[0][CANARY:-CANARY].reshape(nt, n)
    codes = host[1][CANARY:-CANARY].view(np.uint32).reshape(nt, n)
    rounds = host[2][CANARY:-CANARY].view(np.uint32)
    return lens, codes, rounds


@pytest.mark.parametrize("n,max_bits", T.ALPHABETS)
def test_wave_code_construction_equals_the_serial_routines(codes_ctx, f3, n, max_bits):  # noqa: F811
    """Every table of the generator in ONE launch (500 to 900 waves): lengths, codes and trees built, table by table."""
    tabs = T.tables(n, max_bits)
    freq = np.stack([t for _, _, t in tabs])
    want_lens, want_codes, want_rounds, _ = serial_tables(f3, n, max_bits, tabs)
    assert (want_rounds >= 2).sum() >= 100 and (want_rounds >= 3).sum() >= 50  # the limiter is what this is about
    lens, codes, rounds = device_tables(codes_ctx, n, max_bits, freq)
    bad = [tabs[i][0] for i in range(len(tabs))
           if rounds[i] != want_rounds[i] or not np.array_equal(lens[i], want_lens[i]) or not np.array_equal(codes[i], want_codes[i])]
    print("%d/%d: %d tables, %d rebuilt, %d differ" % (n, max_bits, len(tabs), int((want_rounds >= 2).sum()), len(bad)))
    assert not bad, (len(bad), bad[:8])


def test_wave_code_construction_with_320_symbols_and_odd_counts(codes_ctx, f3):  # noqa: F811
    """The entry's own limits: every lane's five slots full (320 symbols), symbol counts that are no multiple of the
    wave (1, 2, 63, 65, 257), one table and many, and the arguments it must refuse."""
    from snappy_amd import _lib
    rng = np.random.default_rng(T.SEED + 7)
    for n, max_bits, nt in ((320, 15, 40), (320, 9, 40), (1, 1, 3), (2, 1, 3), (63, 6, 5), (65, 7, 5), (257, 15, 1), (128, 7, 9)):
        freq = rng.zipf(1.2, size=(nt, n)).astype(np.float64)
        freq = np.minimum(freq * rng.choice([1, 50, 70000], size=(nt, 1)), 0xffffffff).astype(np.uint32)
        freq[rng.random((nt, n)) < 0.2] = 0
        k = min(n, max_bits + 6)
        freq[0, :] = 0
        freq[0, n - k:] = T.fib(k)  # a ladder that must be rebuilt, in the last slots
        tabs = [("%d/%d #%d" % (n, max_bits, i), None, freq[i]) for i in range(nt)]
        want_lens, want_codes, want_rounds, _ = serial_tables(f3, n, max_bits, tabs)
        lens, codes, rounds = device_tables(codes_ctx, n, max_bits, freq)
        assert np.array_equal(rounds, want_rounds) and np.array_equal(lens, want_lens) and np.array_equal(codes, want_codes), (n, max_bits)
        for i in range(min(nt, 4)):  # (the serial routine is held against the reference at 286, 30 and 19 symbols elsewhere; here too)
            T.check_table(tabs[i][0], freq[i], max_bits, lens[i], codes[i], rounds[i])
    torch = _torch()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for n, max_bits in ((0, 15), (321, 15), (19, 4), (19, 0), (30, 16)):
        with pytest.raises(_lib.SnaphashError) as ei:
            codes_ctx.deflate_codes_device(buf.data_ptr(), 1, n, max_bits, buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
        assert ei.value.code == _lib.EINVAL
    codes_ctx.deflate_codes_device(0, 0, 19, 7, 0, 0, 0)  # no tables: nothing to do


@pytest.fixture(scope="module")
def compressors(built_lib):
    """Context per (staging piece, search depth) the inputs ask for."""
    from snappy_amd import Context
    made = {}

    def get(piece, depth):
        if (piece, depth) not in made:
            made[(piece, depth)] = Context(staging_bytes=piece, deflate_depth=depth)
        return made[(piece, depth)]
    yield get
    for c in made.values():
        c.close()


def test_compressor_edges_equal_the_cpu_model(compressors, f3):  # noqa: F811
    """Every edge input: gzip reads the GPU's member back, and its bytes are the serial model's at the same staging piece
    and at the search depth the library documents for the one asked (a depth of 1 is raised to 4: whole batches of links)."""
    cases = E.edge_inputs()
    assert {c.depth for c in cases.values()} == {0, 1, 128} and {c.piece for c in cases.values()} == {E.CHUNK, E.PIECE}
    for name, c in cases.items():
        gz = compressors(c.piece, c.depth).gzip_buffer(c.data)
        assert gzip.decompress(gz) == c.data, name
        n = ctypes.c_size_t()
        p = f3.f3_model_gzip3(c.data, len(c.data), c.piece, E.effective_depth(c.depth), ctypes.byref(n))
        model = ctypes.string_at(p, n.value)
        f3.f3_free(p)
        assert gz == model, (name, len(gz), len(model))
        st = compressors(c.piece, c.depth).targz_stats()
        assert st["tar_bytes"] == len(c.data) and st["gz_bytes"] == len(gz)
