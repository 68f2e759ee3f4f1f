"""From the bytes of a survey's text files to its x, y, z table: `ascii_to_xyz` (reference data_prep.py:259-336).

The reference reads a PDAL-style pipeline JSON, runs `pandas.read_csv(f, sep=sep, header=skip, names=names, usecols=usecols,
na_values=na_values)` over the files it names, drops the rows with a NaN, applies one column arithmetic (`converters`), drops
`dropcols`, sorts the three remaining columns by name into x, y, z and reprojects.  Here the text is uploaded as bytes and parsed on
the GPU (dbm_text_count_lines, dbm_text_parse, dbm_text_columns in include/dbm.h; text.hip), so with download=False a survey goes from
its files to a resident `DevicePoints` -- and on through `get_region` and `xyz_to_grid` -- without a host table in between:

    points = ascii_to_xyz("highres/20xx_Antarctica_DC8.json", download=False)
    region = get_region(points)
    grid, geometry = xyz_to_grid(points, region)

With download=True the result is an (n, 3) float64 array; the package imports no pandas: `pd.DataFrame(a, columns=list("xyz"))`.

The dialect is defined completely in DESIGN.md "Reading text tables" and checked bit for bit against pandas on the reference's eleven
survey formats (tests/test_ascii_host.py).  What differs from pandas, on purpose: quote characters are NOT interpreted; `na_values`
are compared byte for byte (pandas also matches -9999 against -9999.0); a used field that is neither a number, an infinity nor an NA
string raises ValueError with its line and column at once (pandas hands back an `object` column that fails later), and so does a line
with more fields than names.  Numbers are correctly rounded -- the bits of Python's `float()`: the device converts those it can convert
exactly in one IEEE operation and hands the rest (more than 19 digits, a mantissa above 2^53, a decimal exponent beyond +-22) to
`float()` on the host, row by row.  Files are read in sorted order (the reference: `glob.glob` order, which only permutes rows).
No CPU fallback: without a GPU every call that computes raises DbmError.
"""
import ctypes as C
import glob
import json
import os
import re
import zipfile
from collections import namedtuple

import numpy as np

from . import _lib
from .gridding import SRS_PAIRS, reproject
from .resident import DevicePoints, devptr

# include/dbm.h: bytes of text per workgroup, its threads, the separator value of `\s+` and the limits of a reader description.
# tests/test_ascii_host.py holds them to the header.
TEXT_TILE_BYTES = 16384
TEXT_THREADS = 256
TEXT_SEP_WHITESPACE = 256
TEXT_MAX_FIELDS = 64
TEXT_MAX_NA = 8
TEXT_MAX_NA_BYTES = 16

WHITESPACE = "\\s+"   # the separator string that stands for runs of spaces and tabs
# pandas' default NA strings (pandas._libs.parsers.STR_NA_VALUES)
DEFAULT_NA = ("", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA", "NULL",
              "NaN", "None", "n/a", "nan", "null")

# separator: ',', '\t' or WHITESPACE; skip: `header=skip`; names: every column of the file; usecols: the names parsed; na_values: tuple
# of extra NA strings; converter: (new, a, op, b) for `new = a op b` or None; dropcols: names removed after the converter; filename: glob
# pattern beside the pipeline file (None for a reader built by hand)
TextReader = namedtuple("TextReader", "separator skip names usecols na_values converter dropcols filename",
                        defaults=((), None, (), None))

_NUMBER = re.compile(rb"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?")
_INF = re.compile(rb"[+-]?(?:inf|infinity)", re.IGNORECASE)
_CONVERTER = re.compile(r"\s*([A-Za-z_]\w*)\s*([+-])\s*([A-Za-z_]\w*)\s*")


def check_reader(reader):
    """The reader description, validated and normalised (tuples, na_values a tuple of str).  ValueError for anything the dialect does
    not cover."""
    sep = reader.separator
    if sep not in (",", "\t", WHITESPACE):
        raise ValueError(f"the separator must be ',', a tab or {WHITESPACE!r}, got {sep!r}")
    skip = reader.skip
    if isinstance(skip, bool) or int(skip) != skip or int(skip) < 0 or int(skip) >= 2 ** 31 - 1:
        raise ValueError(f"skip must be a non-negative integer, got {skip!r}")
    names, usecols = tuple(reader.names), tuple(reader.usecols)
    if not 1 <= len(names) <= TEXT_MAX_FIELDS or len(set(names)) != len(names) or not all(isinstance(n, str) and n for n in names):
        raise ValueError(f"header must hold 1..{TEXT_MAX_FIELDS} distinct names, got {names!r}")
    unknown = [c for c in usecols if c not in names]
    if unknown:
        raise ValueError(f"usecols names {unknown!r}, which the header {names!r} does not hold")
    if not usecols or len(set(usecols)) != len(usecols):
        raise ValueError(f"usecols must hold distinct names, at least one; got {usecols!r}")
    na = reader.na_values
    na = () if na is None else ((na,) if isinstance(na, str) else tuple(na))
    for s in na:
        if not isinstance(s, str) or not 1 <= len(s.encode()) <= TEXT_MAX_NA_BYTES or "\0" in s or s != s.strip(" \t"):
            raise ValueError(f"an na_values string must hold 1..{TEXT_MAX_NA_BYTES} bytes and no outer blanks, got {s!r}")
    if len(na) > TEXT_MAX_NA:
        raise ValueError(f"at most {TEXT_MAX_NA} na_values strings are supported, got {len(na)}")
    columns = [n for n in names if n in usecols]
    conv = reader.converter
    if conv is not None:
        new, a, op, b = conv
        if op not in ("+", "-") or a not in columns or b not in columns or not isinstance(new, str) or not new:
            raise ValueError(f"the converter must be NEW = A + B or A - B over used columns, got {conv!r}")
        conv = (new, a, op, b)
        columns = [c for c in columns if c != new] + [new]
    drop = tuple(reader.dropcols or ())
    missing = [c for c in drop if c not in columns]
    if missing:
        raise ValueError(f"dropcols names {missing!r}, which are not among the columns {columns!r}")
    return TextReader(sep, int(skip), names, usecols, na, conv, drop, reader.filename)


def table_columns(reader):
    """The used names in file order: the columns of `read_text_table`'s table"""
    return [n for n in reader.names if n in reader.usecols]


def xyz_plan(reader):
    """After the read (data_prep.py:307-320): [(a, op, b), ...] for x, y, z -- column indices into the table, op '+', '-' or None
    (b unused).  ValueError unless exactly three columns remain."""
    cols = table_columns(reader)
    source = {c: (cols.index(c), None, 0) for c in cols}
    if reader.converter is not None:
        new, a, op, b = reader.converter
        source[new] = (cols.index(a), op, cols.index(b))
    for c in reader.dropcols:
        del source[c]
    if len(source) != 3:
        raise ValueError(f"exactly three columns must remain for x, y, z; got {sorted(source)!r}")
    return [source[c] for c in sorted(source)]


def parse_pipeline(pipeline_file):
    """(TextReader, (in_srs, out_srs) or None) of a PDAL-style pipeline JSON (data_prep.py:280-296, 322-326): its `readers.text` stage
    {filename, separator, skip, header, usecols[, na_values, converters, dropcols]} -- header, usecols and dropcols are names joined by
    the separator string -- and its optional `filters.reprojection` stage.  Everything is validated here, on the host; `converters`
    must be one entry {NEW: "A+B"} or {NEW: "A-B"} (the reference evaluates it with DataFrame.eval; nothing is evaluated here)."""
    pipeline_file = os.fspath(pipeline_file)
    if not pipeline_file.endswith(".json"):
        raise ValueError(f"the pipeline file must be a .json file, got {pipeline_file!r}")
    with open(pipeline_file) as f:
        stages = json.load(f)["pipeline"]
    by_type = {s["type"]: s for s in stages}
    if "readers.text" not in by_type:
        raise ValueError(f"{pipeline_file}: no readers.text stage")
    r = by_type["readers.text"]
    for key in ("filename", "separator", "skip", "header", "usecols"):
        if key not in r:
            raise ValueError(f"{pipeline_file}: readers.text lacks {key!r}")
    sep = r["separator"]
    if not isinstance(sep, str) or not sep:
        raise ValueError(f"{pipeline_file}: the separator must be a string, got {sep!r}")
    conv = None
    if "converters" in r:
        entries = r["converters"]
        if not isinstance(entries, dict) or len(entries) != 1:
            raise ValueError(f"{pipeline_file}: converters must hold exactly one entry, got {entries!r}")
        (new, expr), = entries.items()
        m = _CONVERTER.fullmatch(expr) if isinstance(expr, str) else None
        if m is None:
            raise ValueError(f"{pipeline_file}: the converter must be 'A+B' or 'A-B' of two column names, got {expr!r}")
        conv = (new, m.group(1), m.group(2), m.group(3))
    reader = check_reader(TextReader(sep, r["skip"], r["header"].split(sep), r["usecols"].split(sep), r.get("na_values"), conv,
                                     r["dropcols"].split(sep) if "dropcols" in r else (), r["filename"]))
    xyz_plan(reader)
    srs = None
    if "filters.reprojection" in by_type:
        p = by_type["filters.reprojection"]
        srs = (str(p["in_srs"]), str(p["out_srs"]))
        if (srs[0].upper(), srs[1].upper()) not in SRS_PAIRS:
            raise ValueError(f"{pipeline_file}: only {sorted(SRS_PAIRS)} can be reprojected, got {srs[0]!r} -> {srs[1]!r}")
    return reader, srs


# ---- one line on the host: what the device leaves to float(), and the wording of errors ----
def _fields(line, sep):
    if sep == WHITESPACE:
        return [f for f in re.split(rb"[ \t]+", line) if f]
    return line.split(sep.encode())


def _host_row(line, reader, where):
    """The used fields of one non-blank line (bytes without its line end) as floats, NaN included; ValueError names `where` and the
    column"""
    fields = _fields(line, reader.separator)
    if len(fields) > len(reader.names):
        raise ValueError(f"{where}: {len(fields)} fields, the header names {len(reader.names)}")
    na = set(s.encode() for s in DEFAULT_NA + reader.na_values)
    row = []
    for k, name in enumerate(reader.names):
        if name not in reader.usecols:
            continue
        f = fields[k].strip(b" \t") if k < len(fields) else b""
        if f in na:
            row.append(float("nan"))
        elif _INF.fullmatch(f) or _NUMBER.fullmatch(f):
            row.append(float(f.decode("ascii")))
        else:
            raise ValueError(f"{where}: column {name!r}: {f[:40]!r} is neither a number nor an NA string")
    return row


def _line_at(buf, off):
    """the bytes of the line that starts at byte `off` of the uint8 array, without '\\n' or '\\r\\n'"""
    end, step = off, 1 << 16
    while True:
        hit = np.flatnonzero(buf[end:end + step] == 10)
        if hit.size or end + step >= buf.size:
            end = end + int(hit[0]) if hit.size else buf.size
            break
        end += step
    line = buf[off:end].tobytes()
    return line[:-1] if end < buf.size and line.endswith(b"\r") else line


def _bytes_array(data):
    if isinstance(data, (str, os.PathLike)):
        return np.fromfile(os.fspath(data), dtype=np.uint8)
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    arr = np.asarray(data)
    if arr.dtype != np.uint8 or arr.ndim != 1:
        raise ValueError(f"data must be bytes, a one-dimensional uint8 array or a path; got {arr.dtype} {arr.shape}")
    return np.ascontiguousarray(arr)


def _separator_code(sep):
    return TEXT_SEP_WHITESPACE if sep == WHITESPACE else ord(sep)


def _read_resident(buf, reader, ctx):
    """The table of one file's bytes as a DevicePoints of the used columns, which owns it; without a row it owns nothing (ptr 0)"""
    names = reader.names
    nuse = len(reader.usecols)
    empty = DevicePoints.adopt(0, 0, nuse, ctx)
    if buf.size == 0:
        return empty
    mask = sum(1 << k for k, n in enumerate(names) if n in reader.usecols)
    na = b"".join(s.encode() + b"\0" for s in reader.na_values)
    sep = _separator_code(reader.separator)
    with ctx.scratch(buf.size + 16) as text:
        ctx.upload(text, buf)
        counts = (C.c_int64 * 2)()
        ctx.call("dbm_text_count_lines", devptr(text), buf.size, sep, counts, _lib.DEVICE_PTRS)
        cap = max(int(counts[1]) - reader.skip - 1, 0)   # every non-blank line behind the discarded ones may be a row
        if cap == 0:
            return empty
        table = DevicePoints.adopt(ctx.malloc(8 * nuse * cap), 0, nuse, ctx)
        repair = np.empty((cap, 2), dtype=np.int64)      # (untouched pages cost nothing)
        result = (C.c_int64 * 4)()
        ctx.call("dbm_text_parse", devptr(text), buf.size, sep, reader.skip, len(names), mask, na, len(reader.na_values), devptr(table), cap,
                 devptr(repair), cap, result, _lib.DEVICE_PTRS)
        table.n, nrep, bad = int(result[0]), int(result[1]), int(result[2])
        if bad >= 0:
            where = f"line {int(np.count_nonzero(buf[:bad] == 10)) + 1}"
            _host_row(_line_at(buf, bad), reader, where)
            raise ValueError(f"{where}: cannot be parsed")   # (the device and the host disagree: not reachable by design)
        for off, row in repair[:nrep]:
            vals = np.array(_host_row(_line_at(buf, int(off)), reader, f"byte {int(off)}"), dtype=np.float64)
            ctx.upload(table.ptr + 8 * nuse * int(row), vals)
        return table if table.n else empty


def read_text_table(data, reader, download=True, ctx=None):
    """`pandas.read_csv(data, sep, header=skip, names, usecols, na_values).dropna()` (data_prep.py:298-305) of ONE file.  data: bytes, a
    one-dimensional uint8 array, or a path; reader: a TextReader (its converter, dropcols and filename are not used here).  Returns
    (table (n, nuse) float64, column names): the used columns in file order, the kept rows in file order -- or, with download=False, a
    `DevicePoints` of nuse columns in place of the array.  ValueError names the first line in the file that cannot be parsed (1-based)
    and, for a bad field, its column."""
    reader = check_reader(reader)
    buf = _bytes_array(data)
    ctx = ctx or _lib.default_context()
    table = _read_resident(buf, reader, ctx)
    cols = table_columns(reader)
    if not download:
        table.ptr = table.ptr or ctx.malloc(8)
        return table, cols
    return ctx.download(table.ptr, np.float64, (table.n, table.ncol)), cols


def _file_bytes(path):
    """the file's bytes; a .zip with exactly one member is inflated (host, zipfile)"""
    if path.lower().endswith(".zip"):
        with zipfile.ZipFile(path) as z:
            members = [m for m in z.namelist() if not m.endswith("/")]
            if len(members) != 1:
                raise ValueError(f"{path}: a .zip must hold exactly one file, it holds {len(members)}")
            return np.frombuffer(z.read(members[0]), dtype=np.uint8)
    return np.fromfile(path, dtype=np.uint8)


def ascii_to_xyz(pipeline_file, download=True, ctx=None):
    """ascii_to_xyz (data_prep.py:259-336): the files matching the pipeline's `filename` beside the pipeline file, in SORTED order (the
    reference: `glob.glob` order -- the same rows, permuted by file), each read as `read_text_table` reads it, concatenated; the
    converter and dropcols applied, the three remaining columns sorted by name into x, y, z (one launch per file, on the device: the
    converter is ONE IEEE addition or subtraction); a `filters.reprojection` stage reprojects the resident table (`reproject`).
    Returns (n, 3) float64 x, y, z -- `pd.DataFrame(a, columns=list("xyz"))` gives the reference's frame -- or with download=False a
    `DevicePoints`, which `get_region`, `blockmedian` and `xyz_to_grid` use in place."""
    reader, srs = parse_pipeline(pipeline_file)
    plan = xyz_plan(reader)
    pattern = os.path.join(os.path.dirname(os.fspath(pipeline_file)), reader.filename)
    files = sorted(glob.glob(pattern))
    if not files:
        raise ValueError(f"no file matches {pattern!r}")
    ctx = ctx or _lib.default_context()
    parts = []
    for path in files:
        try:
            parts.append(_read_resident(_file_bytes(path), reader, ctx))
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None
    n = sum(len(part) for part in parts)
    if n >= 2 ** 31:
        raise ValueError(f"{n} rows: a point table must stay below 2^31 rows")
    points = DevicePoints.adopt(ctx.malloc(max(24 * n, 8)), n, 3, ctx)
    a = (C.c_int * 3)(*[p[0] for p in plan])
    b = (C.c_int * 3)(*[p[2] for p in plan])
    op = (C.c_int * 3)(*[{None: 0, "+": 1, "-": 2}[p[1]] for p in plan])
    at = 0
    for part in parts:
        if len(part):
            ctx.call("dbm_text_columns", devptr(part), part.n, part.ncol, devptr(points.ptr + 24 * at), 3, a, op, b)
        at += len(part)
    ctx.synchronize()
    if srs is not None and n:
        reproject(points, srs[0], srs[1])
    if not download:
        return points
    return ctx.download(points.ptr, np.float64, (n, 3))
