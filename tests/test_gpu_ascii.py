"""-m gpu: dbm_text_count_lines, dbm_text_parse and dbm_text_columns (reference data_prep.py:259-336, ascii_to_xyz) through the C ABI and
through deepbedmap_amd/ascii_table.py, against the pure-Python restatement (tests/ascii_restatement.py, pinned bit for bit to pandas
and to float() in tests/test_ascii_host.py).

Every comparison with the restatement is BIT FOR BIT: a field is either converted by one IEEE operation on exact operands or by
float() itself, the converter is one IEEE subtraction, rows are kept in file order.  The one exception is the reprojection, which keeps
the bound of tests/test_gpu_gridding.py: |delta| <= 1e-6 m against gridding_restatement (derived there)."""
import ctypes as C
import os
import sys
import time
import zipfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ascii_restatement as ar  # noqa: E402
import gridding_restatement as gr  # noqa: E402
from test_ascii_host import BAD, FORMAT_IDS, FORMATS, INFINITIES, NUMBERS, make_file, same_bits, write_pipeline  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


@pytest.fixture(scope="module")
def T():
    from deepbedmap_amd import ascii_table

    return ascii_table.TEXT_TILE_BYTES


def agree(dbm, data, sep, skip, names, usecols, na=()):
    """the device's table of `data` equals the restatement's, bit for bit; returns it"""
    want, wcols = ar.read_table(data, sep, skip, names, usecols, na)
    got, cols = dbm.read_text_table(data, dbm.TextReader(sep, skip, names, usecols, na))
    assert cols == wcols
    assert got.shape == want.shape, (got.shape, want.shape)
    assert same_bits(got, want)
    return got


ABC = ["a", "b", "c"]


def filler_file(first_newline_at, tail_lines=40):
    """'h', then a line '1.5,2.5,xxx...' whose '\\n' sits at byte `first_newline_at`, then short lines with distinct values"""
    head = b"h\n1.5,2.5,"
    data = head + b"x" * (first_newline_at - len(head)) + b"\n"
    assert data.index(b"\n", 2) == first_newline_at
    return data + b"".join(b"%d.25,-%d.5,q%d\n" % (k, k, k) for k in range(tail_lines))


# ---- the eleven formats through ascii_to_xyz ----
@pytest.mark.parametrize("k", range(len(FORMATS)), ids=FORMAT_IDS)
def test_eleven_formats_through_ascii_to_xyz(dbm, tmp_path, k):
    fmt = FORMATS[k]
    tables = []
    for j, name in enumerate(sorted(fmt["files"])):
        data = make_file(fmt, seed=1000 + 10 * k + j, final_newline=(k + j) % 2 == 1)
        path = os.path.join(str(tmp_path), name)
        if name.endswith(".zip"):
            with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
                z.writestr(name[:-4] + ".txt", data)
        else:
            with open(path, "wb") as f:
                f.write(data)
        tables.append(ar.read_table(data, fmt["separator"], fmt["skip"], fmt["header"], fmt["usecols"], fmt["na_values"]))
    cols = tables[0][1]
    want = ar.to_xyz(np.concatenate([t for t, _ in tables]), cols, fmt["converter"], fmt["dropcols"])
    pipeline = write_pipeline(fmt, tmp_path)
    got = dbm.ascii_to_xyz(pipeline)
    assert got.shape == want.shape and len(got) > 150 * len(fmt["files"])
    resident = dbm.ascii_to_xyz(pipeline, download=False)
    assert isinstance(resident, dbm.DevicePoints) and (resident.n, resident.ncol) == want.shape
    if fmt["reprojection"]:
        ref = gr.polar_stereographic(want)
        worst = float(np.abs(got[:, :2] - ref[:, :2]).max())
        print(f"{fmt['name']}: reprojection worst |delta| = {worst:.3e} m")
        assert worst <= 1e-6
        assert same_bits(got[:, 2], want[:, 2])
    else:
        assert same_bits(got, want)


# ---- tile edges ----
@pytest.mark.parametrize("delta", [-2, -1, 0, 1, 2])
def test_newline_around_a_tile_edge(dbm, T, delta):
    agree(dbm, filler_file(T + delta), ",", 0, ABC, ["a", "b"])
    agree(dbm, filler_file(2 * T + delta), ",", 1, ABC, ["a", "b"])


def test_number_straddling_a_tile_edge(dbm, T):
    for before in range(1, 13):   # '123456.789012' starts `before` bytes in front of the edge
        data = filler_file(T - before - 1)
        data = data[:T - before] + b"123456.789012,-0.000123456,tail\n9,8,7\n"
        got = agree(dbm, data, ",", 0, ABC, ["a", "b"])
        assert got[1].tolist() == [123456.789012, -0.000123456]


def test_carriage_return_at_the_end_of_a_tile(dbm, T):
    data = filler_file(T)                        # '\n' at T ...
    data = data[:T - 1] + b"\r" + data[T:]      # ... and '\r' at T - 1
    got = agree(dbm, data, ",", 0, ABC, ["a", "b"])
    assert got[0].tolist() == [1.5, 2.5]
    # the same with the '\r' directly behind a used field
    data = b"h\n" + b"7,8," + b"x" * (T - 20) + b"\n"
    data += b" " * (T - 1 - len(data) - 8) + b"1.5,2.25\r\n3,4\r\n"
    assert data[T - 1:T + 1] == b"\r\n"
    got = agree(dbm, data, ",", 0, ["a", "b"] + ["c"], ["a", "b"])
    assert got[1].tolist() == [1.5, 2.25]


def test_a_line_spanning_three_tiles(dbm, T):
    names = ["a", "b", "c", "d"]
    long_line = b"1.5,2.5," + b"x" * (2 * T + 100) + b",7.125\n"
    data = b"h\n" + b"9,9,9,9\n" * 700 + long_line + b"3,4,q,5\n" * 3 + long_line.replace(b"7.125", b"-8e3") + b"6,7,q,8"
    start = data.index(long_line)
    assert start // T + 2 == (start + len(long_line) - 8) // T     # its last, used field begins in the third tile of the line
    got = agree(dbm, data, ",", 0, names, ["a", "b", "d"])
    assert got[700].tolist() == [1.5, 2.5, 7.125] and got[704].tolist() == [1.5, 2.5, -8000.0]
    # whitespace-separated, and the line longer than the tile is the last one, without a newline
    ws = b"h\n" + b"1 2 3\n" * 10 + b"4   " + b"x" * (T + 50) + b" \t 6.5"
    agree(dbm, ws, ar.WHITESPACE, 0, ABC, ["a", "c"])


# ---- file sizes ----
def test_tiny_and_exact_sizes(dbm, T):
    one = ["a"]
    for data in (b"", b"\n", b"5", b"\n\n \n", b"h\n", b"h", b"h\r\n"):
        assert agree(dbm, data, ",", 0, one, one).shape == (0, 1)
    assert agree(dbm, b"h\n5", ",", 0, one, one).tolist() == [[5.0]]
    assert agree(dbm, b"5", ",", 0, ["a", "b"], ["a", "b"]).shape == (0, 2)
    for size in (T - 1, T, T + 1, 2 * T):
        for newline in (True, False):
            body = b"h\n" + b"1.5,2.5\n" * (size // 8 + 1)
            data = body[:size - 12] + b"\n" + b" " * 20
            data = data[:size - 5] + (b"7,-8\n" if newline else b",7,-8")
            assert len(data) == size
            got = agree(dbm, data, ",", 0, ABC, ["a", "b"])
            assert len(got) > size // 8 - 4
    lines = b"h\n" + b"1,2\n" * 10
    for skip in (9, 10, 11, 1000):
        assert agree(dbm, lines, ",", skip, ["a", "b"], ["a", "b"]).shape == (max(10 - skip, 0), 2)


# ---- lanes: lines per tile against threads per workgroup ----
def test_lines_per_tile(dbm, T):
    from deepbedmap_amd import ascii_table

    threads = ascii_table.TEXT_THREADS
    for per_tile in (1, 63, 64, 65, threads - 1, threads, threads + 1, 4 * threads):
        length = T // per_tile
        lines = []
        for k in range(3 * per_tile + 2):
            core = b"%d.5,%d," % (k, -k)
            lines.append(core + b"x" * max(length - len(core) - 1, 0) + b"\n")
        got = agree(dbm, b"h\n" + b"".join(lines), ",", 0, ABC, ["a", "b"])
        assert len(got) == 3 * per_tile + 2
    # nothing but newlines, and nothing but one-byte lines: 64 line starts in every thread's bytes
    assert agree(dbm, b"\n" * (T + 5), ",", 0, ["a"], ["a"]).shape == (0, 1)
    got = agree(dbm, b"h\n" + b"7\n" * (T + 5), ",", 0, ["a"], ["a"])
    assert got.shape == (T + 5, 1) and (got == 7.0).all()


# ---- grammar ----
def test_grammar_through_the_device(dbm):
    na = ("*", "-9999", "missing")
    texts = NUMBERS + INFINITIES + list(ar.DEFAULT_NA) + list(na) + ["-9999.0", "  12.5  ", "\t-3e2 "]
    data = "v,k\n" + "".join(f"{t},{k}\n" for k, t in enumerate(texts))
    got = agree(dbm, data.encode(), ",", 0, ["v", "k"], ["v", "k"], na)
    kept = [k for k, t in enumerate(texts) if t.strip() not in ar.DEFAULT_NA + na]
    assert got[:, 1].tolist() == [float(k) for k in kept]
    for k, v in zip(kept, got[:, 0]):
        assert same_bits(np.array([v]), np.array([float(texts[k])])), texts[k]
    # the same fields separated by tabs and by runs of blanks (no empty field, no field with a blank inside)
    plain = [t.strip() for t in texts if t.strip() and " " not in t.strip()]
    agree(dbm, ("v\tk\n" + "".join(f"{t}\t{k}\n" for k, t in enumerate(plain))).encode(), "\t", 0, ["v", "k"], ["v", "k"], na)
    agree(dbm, ("v k\n" + "".join(f" {t} \t {k}\n" for k, t in enumerate(plain))).encode(), ar.WHITESPACE, 0, ["v", "k"], ["v", "k"], na)


@pytest.mark.parametrize("text", BAD)
def test_bad_fields_raise_through_the_device(dbm, text):
    reader = dbm.TextReader("\t", 0, ["v", "k"], ["v", "k"])
    data = ("v\tk\n1\t0\n" + text + "\t1\n").encode()
    with pytest.raises(ValueError, match="line 3: column 'v'"):
        dbm.read_text_table(data, reader)
    with pytest.raises(ValueError, match="line 3: column 'v'"):
        ar.read_table(data, "\t", 0, ["v", "k"], ["v", "k"])


def test_a_file_of_nothing_but_host_repair_fields(dbm):
    rng = np.random.default_rng(7)
    lines = []
    for k in range(1500):
        a = "%.25f" % rng.uniform(-1.0, 1.0)                        # more than 19 significant digits
        b = "%d.%de-%d" % (rng.integers(1, 9), rng.integers(1, 10 ** 9), rng.integers(23, 330))    # an exponent beyond -22
        c = "%d" % rng.integers(2 ** 53 + 1, 2 ** 63)               # a mantissa above 2^53
        lines.append(f"{a},{b},{c}\n")
    got = agree(dbm, ("a,b,c\n" + "".join(lines)).encode(), ",", 0, ABC, ABC)
    assert got.shape == (1500, 3)
    # a few of them among ordinary rows, some of those rows dropped
    mixed = "a,b,c\n" + "".join(lines[k // 7] if k % 7 == 3 else ("NaN,1,2\n" if k % 5 == 0 else f"{k}.5,{-k},1e3\n") for k in range(3000))
    agree(dbm, mixed.encode(), ",", 0, ABC, ABC)


# ---- dropping and order ----
def test_dropping_keeps_file_order_and_is_deterministic(dbm):
    rng = np.random.default_rng(11)
    n = 20000
    drop = rng.random(n) < 1.0 / 3.0
    rows = []
    for k in range(n):
        x, y, z = "%.6f" % rng.uniform(-180, 180), "%.6f" % rng.uniform(-90, -60), "%.2f" % rng.uniform(-3000, 3000)
        if drop[k]:
            which = int(rng.integers(0, 3))
            x, y, z = [("NaN" if j == which else v) for j, v in enumerate((x, y, z))]
        rows.append(f"{x},{y},{k},{z}\n")
    names = ["x", "y", "k", "z"]
    data = ("x,y,k,z\n" + "".join(rows)).encode()
    got = agree(dbm, data, ",", 0, names, names)
    assert got[:, 2].tolist() == [float(k) for k in range(n) if not drop[k]]
    again, _ = dbm.read_text_table(data, dbm.TextReader(",", 0, names, names))
    assert same_bits(got, again)
    none = ("x,y,k,z\n" + "".join(f"1,2,{k},3\n" for k in range(n))).encode()
    assert len(agree(dbm, none, ",", 0, names, names)) == n
    every = ("x,y,k,z\n" + "".join(f"1,,{k},3\n" for k in range(n))).encode()
    assert agree(dbm, every, ",", 0, names, names).shape == (0, 4)


def test_compaction_past_one_round_of_the_tile_scan(dbm):
    """256 * 2048 + 1 candidates: 257 scan tiles of the flag bytes, so the one-workgroup pass over the tiles' sums takes a second round
    and the compaction's rescan adds a base that round produced (candidate 524 288, alone in the last tile, is a host-repair row: both
    of its bases, rows kept and rows for the host, come from there).  Against the table built from k directly."""
    n = 256 * 2048 + 1
    repair = {100001: ("0.1234567890123456789012345", "1.5e-30", "9007199254740993"),     # too many digits, exponent beyond -22,
              300000: ("-0.9876543210987654321098765", "2.25e-300", "18014398509481985"),  # mantissa above 2^53
              n - 1: ("0.5000000000000000000000001", "7.125e-23", "9007199254740995")}
    assert all(k % 7 for k in repair)
    lines = ["NaN,1,2\n" if k % 7 == 0 else f"{k}.5,{-k},1e3\n" for k in range(n)]
    for k, fields in repair.items():
        lines[k] = ",".join(fields) + "\n"
    data = ("a,b,c\n" + "".join(lines)).encode()
    k = np.arange(n, dtype=np.int64)
    want = np.stack([k + 0.5, (-k).astype(np.float64), np.full(n, 1e3)], axis=1)
    for at, fields in repair.items():
        want[at] = [float(f) for f in fields]
    want = want[k % 7 != 0]
    got, cols = dbm.read_text_table(data, dbm.TextReader(",", 0, ABC, ABC))
    assert list(cols) == ABC and got.shape == want.shape, (cols, got.shape, want.shape)
    assert same_bits(got, want)
    again, _ = dbm.read_text_table(data, dbm.TextReader(",", 0, ABC, ABC))
    assert same_bits(got, again)


# ---- errors ----
def test_errors_name_the_first_line_in_the_file(dbm, T):
    good = b"1.5,2.5,junk\n"
    n = 3 * T // len(good)
    lines = [good] * n
    lines[n - 5] = b"1.5,oops,junk\n"           # in the third tile
    lines[n // 2] = b"1.5,2.5.5,junk\n"         # in the second: the first in the file
    data = b"a,b,c\n\n" + b"".join(lines)
    reader = dbm.TextReader(",", 0, ABC, ["a", "b"])
    with pytest.raises(ValueError, match=rf"line {n // 2 + 3}: column 'b'"):
        dbm.read_text_table(data, reader)
    with pytest.raises(ValueError, match=rf"line {n // 2 + 3}: column 'b'"):
        ar.read_table(data, ",", 0, ABC, ["a", "b"])
    lines[n // 2] = good
    with pytest.raises(ValueError, match=rf"line {n - 5 + 3}: column 'b'"):
        dbm.read_text_table(data.replace(b"2.5.5", b"2.5"), reader)
    # junk in an unused field is accepted; bad fields in the discarded lines are nobody's business
    agree(dbm, b"junk,junk,junk\n" + b"".join(lines).replace(b"oops", b"3") + b"4,5,\"6\"\n", ",", 0, ABC, ["a", "b"])
    # more fields than names
    with pytest.raises(ValueError, match=r"line 3: 4 fields"):
        dbm.read_text_table(b"a,b,c\n1,2,3\n1,2,3,4\n", reader)
    with pytest.raises(ValueError, match=r"line 2: 4 fields"):
        dbm.read_text_table(b"h\n1 2 3 4\n", dbm.TextReader(ar.WHITESPACE, 0, ABC, ["a"]))


# ---- the C ABI ----
def test_calling_forms_agree_and_refusals(dbm):
    from deepbedmap_amd import _lib

    lib, ctx = _lib.lib(), _lib.default_context()
    data = make_file(FORMATS[3], seed=5, lines=300)
    want, _ = ar.read_table(data, ",", 1, FORMATS[3]["header"], FORMATS[3]["usecols"])
    counts = (C.c_int64 * 2)()
    assert lib.dbm_text_count_lines(ctx.handle, data, len(data), ord(","), counts, 0) == 0
    assert tuple(counts) == ar.count_lines(data, ",")
    mask = sum(1 << k for k, n in enumerate(FORMATS[3]["header"]) if n in FORMATS[3]["usecols"])
    cap = counts[1] - 2
    table, repair, result = np.full((cap, 4), -1.0), np.zeros((cap, 2), dtype=np.int64), (C.c_int64 * 4)()
    args = (table.ctypes.data_as(C.c_void_p), cap, repair.ctypes.data_as(C.c_void_p), cap, result, 0)
    assert lib.dbm_text_parse(ctx.handle, data, len(data), ord(","), 1, 9, mask, None, 0, *args) == 0    # host pointers
    assert tuple(result) == (len(want), 0, -1, cap) and same_bits(table[:len(want)], want) and (table[len(want):] == -1.0).all()

    def refused(rc):
        assert rc == 1 and b"dbm_text_parse" in lib.dbm_last_error(ctx.handle)

    refused(lib.dbm_text_parse(ctx.handle, data, len(data), ord(";"), 1, 9, mask, None, 0, *args))
    refused(lib.dbm_text_parse(ctx.handle, data, len(data), ord(","), -1, 9, mask, None, 0, *args))
    refused(lib.dbm_text_parse(ctx.handle, data, len(data), ord(","), 1, 65, mask, None, 0, *args))
    refused(lib.dbm_text_parse(ctx.handle, data, len(data), ord(","), 1, 9, 0, None, 0, *args))
    refused(lib.dbm_text_parse(ctx.handle, data, len(data), ord(","), 1, 9, 1 << 9, None, 0, *args))
    refused(lib.dbm_text_parse(ctx.handle, data, len(data), ord(","), 1, 9, mask, b"\0", 1, *args))
    refused(lib.dbm_text_parse(ctx.handle, data, len(data), ord(","), 1, 9, mask, b"x" * 17 + b"\0", 1, *args))
    small = (table.ctypes.data_as(C.c_void_p), len(want) - 1, repair.ctypes.data_as(C.c_void_p), cap, result, 0)
    before = table.copy()
    refused(lib.dbm_text_parse(ctx.handle, data, len(data), ord(","), 1, 9, mask, None, 0, *small))
    assert same_bits(table, before)


# ---- the resident chain ----
def test_resident_chain_from_text_to_block_medians(dbm, tmp_path):
    rng = np.random.default_rng(3)
    n, x0, y0 = 5000, -1600000.0, -250000.0
    x, y, z = rng.uniform(x0, x0 + 50 * 250.0, n), rng.uniform(y0 - 40 * 250.0, y0, n), rng.normal(-500.0, 800.0, n)
    text = "x,y,z\n" + "".join(("%.2f,%.2f,%.3f\n" % r) if k % 97 else ("%.2f,NaN,%.3f\n" % (r[0], r[2])) for k, r in enumerate(zip(x, y, z)))
    fmt = FORMATS[9]
    with open(os.path.join(str(tmp_path), fmt["files"][0]), "wb") as f:
        f.write(("preamble\n" + text).encode())
    pipeline = write_pipeline(fmt, tmp_path)
    table, cols = ar.read_table(("preamble\n" + text).encode(), ",", 1, ["x", "y", "z"], ["x", "y", "z"])
    host = ar.to_xyz(table, cols)
    assert len(host) == n - len(range(0, n, 97))
    points = dbm.ascii_to_xyz(pipeline, download=False)
    assert same_bits(dbm.ascii_to_xyz(pipeline), host)
    region = dbm.get_region(points)
    assert region == dbm.get_region(host)
    assert same_bits(dbm.blockmedian(points, region), dbm.blockmedian(host, region))
    H, W = dbm.block_shape(region, 250)
    assert (H, W) == (41, 51)
    grid, geometry = dbm.xyz_to_grid(points, region)
    assert grid.shape == (H - 1, W - 1) and geometry.registration == "pixel" and np.isfinite(grid).any()


# ---- offsets above 4 GiB ----
def test_offsets_above_four_gib(dbm):
    """A 1 MiB block of 256 lines of 4096 bytes, tiled to 2^32 + 2^20 bytes on the device: the smallest input on which a 32-bit byte
    offset wraps (and it crosses 2^31 on the way).  Every row is compared.  Wall time of the two calls: DESIGN.md 6g."""
    from deepbedmap_amd import _lib

    lib, ctx = _lib.lib(), _lib.default_context()
    rng = np.random.default_rng(5)
    lines = []
    for k in range(256):
        head = "%.6f,%s," % (rng.uniform(-180, 180), "NaN" if k % 50 == 7 else "%.6f" % rng.uniform(-90, -60))
        tail = ",%.3f\n" % rng.uniform(-3000, 3000)
        lines.append(head + "f" * (4096 - len(head) - len(tail)) + tail)
    block = "".join(lines).encode()
    assert len(block) == 1 << 20
    names, use = ["a", "b", "fat", "c"], ["a", "b", "c"]
    one, _ = ar.read_table(b"h\n" + block, ",", 0, names, use)          # every line of the block
    first, _ = ar.read_table(block, ",", 0, names, use)                 # the block at the head of the file: its first line discarded
    copies = (1 << 12) + 1
    nbytes = copies * len(block)
    assert nbytes > 2 ** 32
    want = np.concatenate([first, np.tile(one, (copies - 1, 1))])
    text = ctx.malloc(nbytes)
    table = 0
    try:
        src = np.frombuffer(block, dtype=np.uint8)
        for k in range(copies):
            _lib.check(lib.dbm_memcpy_h2d(ctx.handle, C.c_void_p(text + k * len(block)), src.ctypes.data_as(C.c_void_p), len(block)), ctx.handle)
        t0 = time.perf_counter()
        counts = (C.c_int64 * 2)()
        _lib.check(lib.dbm_text_count_lines(ctx.handle, C.c_void_p(text), nbytes, ord(","), counts, _lib.DEVICE_PTRS), ctx.handle)
        assert tuple(counts) == (256 * copies, 256 * copies)
        cap = counts[1] - 1
        table = ctx.malloc(24 * cap)
        result = (C.c_int64 * 4)()
        _lib.check(lib.dbm_text_parse(ctx.handle, C.c_void_p(text), nbytes, ord(","), 0, 4, 0b1011, None, 0, C.c_void_p(table), cap, None, 0,
                                      result, _lib.DEVICE_PTRS), ctx.handle)
        print(f"4 GiB + 1 MiB of text: count + parse took {time.perf_counter() - t0:.3f} s")
        assert tuple(result) == (len(want), 0, -1, cap)
        got = np.empty_like(want)
        _lib.check(lib.dbm_memcpy_d2h(ctx.handle, got.ctypes.data_as(C.c_void_p), C.c_void_p(table), got.nbytes), ctx.handle)
        assert same_bits(got, want)
    finally:
        ctx.free(text)
        if table:
            ctx.free(table)
