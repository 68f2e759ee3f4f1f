"""CPU checks of the text dialect (DESIGN.md "Reading text tables"): tests/ascii_restatement.py -- what dbm_text_parse computes -- against
`pandas.read_csv(...).dropna()` bit for bit on generated files in the eleven formats of the reference's surveys, against `float()` for the
number grammar, and the host-side plumbing of deepbedmap_amd.ascii_table (pipeline validation, constants, bindings, no CPU fallback).
The formats are stated here as a table; the pipeline files are written into tmp_path (none is copied from the reference)."""
import io
import json
import math
import os
import re
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ascii_restatement as ar  # noqa: E402

CRESIS = "Y,X,TIME,THICK,ELEVATION,FRAME,SURFACE,BOTTOM,QUALITY".split(",")
CRESIS_USE = ["X", "Y", "ELEVATION", "BOTTOM"]
LONLAT = ("EPSG:4326", "EPSG:3031")
WISE = ("FlightID Line_name X Y x y Height_WGS1984 Date Time Segy_name traceNum PriNum surfPickLoc bedPickLoc Z Bedrock_and_BEDMAP2 Mask "
        "picked_bedElev surfElev tIce").split()


def _fmt(name, files, pattern, sep, skip, header, usecols, converter=None, dropcols=(), na_values=None, reprojection=None):
    return dict(name=name, files=files, filename=pattern, separator=sep, skip=skip, header=header, usecols=usecols, converter=converter,
                dropcols=tuple(dropcols), na_values=na_values, reprojection=reprojection)


def _cresis(name, files, pattern):
    return _fmt(name, files, pattern, ",", 1, CRESIS, CRESIS_USE, ("Z", "ELEVATION", "-", "BOTTOM"), ("ELEVATION", "BOTTOM"), None, LONLAT)


# the eleven survey formats of the reference (its highres/*.json): separator, skip, header names, usecols, converter, dropcols,
# na_values, reprojection
FORMATS = [
    _fmt("2007tx", ["2007tr.txt", "2007ts.txt"], "2007t?.txt", "\t", 1, "x y z_surf time h h_fc z z_fc".split(), ["x", "y", "z_fc"]),
    _fmt("2010tr", ["2010tr.txt"], "2010tr.txt", "\t", 1, "x y z_surf time h h_fc z_bed z_bed_fc z-surf".split(), ["x", "y", "z_bed_fc"]),
    _cresis("201x_Antarctica_Basler", ["2013_Antarctica_Basler.csv"], "201?_Antarctica_Basler.csv"),
    _cresis("20xx_Antarctica_DC8", ["2014_Antarctica_DC8.csv", "2016_Antarctica_DC8.csv"], "20??_Antarctica_DC8.csv"),
    _cresis("20xx_Antarctica_DC8_THW", ["2009_Antarctica_DC8.csv"], "20??_Antarctica_DC8.csv"),
    _cresis("20xx_Antarctica_TO", ["2011_Antarctica_TO.csv", "2011_Antarctica_TO_b.csv"], "20??_Antarctica_TO*.csv"),
    _cresis("Data_20141121_05", ["Data_20141121_05.csv"], "Data_20141121_05.csv"),
    _fmt("WISE_ISODYN_RadarByFlight", ["WISE_ISODYN_RadarByFlight_ASCII.zip"], "WISE_ISODYN_RadarByFlight_ASCII.zip", ar.WHITESPACE, 11,
         WISE, ["X", "Y", "Z"], na_values="*", reprojection=LONLAT),
    _fmt("bed_WGS84_grid", ["bed_WGS84_grid.txt"], "bed_WGS84_grid.txt", "\t", 20, "x y z column row".split(), ["x", "y", "z"]),
    _fmt("bed_depth_below_WGS84_datum", ["bed_depth_below_WGS84_datum.csv"], "bed_depth_below_WGS84_datum.csv", ",", 1, ["x", "y", "z"],
         ["x", "y", "z"]),
    _fmt("istarxx", ["istar08.txt", "istar18.txt"], "istar??.txt", "\t", 1, "x y z_surf time h h_fc z_bed z_bed_fc".split(),
         ["x", "y", "z_bed_fc"]),
]
FORMAT_IDS = [f["name"] for f in FORMATS]


def _value(rng, fmt, name, k):
    """one printed field of column `name` (column k of the header)"""
    if name == "Y" and fmt["reprojection"]:
        return "%.6f" % rng.uniform(-90.0, -60.0)          # latitude
    if name == "X" and fmt["reprojection"]:
        return "%.6f" % rng.uniform(-180.0, 180.0)         # longitude
    if name not in fmt["usecols"] and k % 3 == 2:
        return rng.choice(["frame_2011", "12:30:01.5", "Data_2014", "n/a?", "--"])    # unused columns may hold anything
    style = (k + int(rng.integers(0, 2))) % 5
    v = rng.uniform(-3000.0, 3000.0)
    return ("%.6f" % v, "%.2f" % v, "%.4f" % v, "%d" % int(v * 100), "%.3e" % (v * 1e3))[style]


def make_file(fmt, seed, lines=400, final_newline=True):
    """bytes of one generated file in format `fmt`: `skip` lines of preamble, then ~`lines` data lines with CRLF on some, blank lines,
    short lines, padded fields, the format's na_values token, NaN"""
    rng = np.random.default_rng(seed)
    sep = fmt["separator"]
    glue = "  " if sep == ar.WHITESPACE else sep
    names = fmt["header"]
    out = []
    for k in range(fmt["skip"]):
        out.append(("# preamble line %d" % k) + "\n")
    out.append(glue.join(names) + "\n")
    na_tokens = ["NaN"] + ([fmt["na_values"]] if fmt["na_values"] else [])
    used = [k for k, n in enumerate(names) if n in fmt["usecols"]]
    for _ in range(lines):
        fields = [_value(rng, fmt, n, k) for k, n in enumerate(names)]
        roll = rng.random()
        if roll < 0.08:
            fields[int(rng.choice(used))] = str(rng.choice(na_tokens))
        elif roll < 0.14:
            fields = fields[:int(rng.integers(1, len(fields)))]             # a short line
        elif roll < 0.24:
            k = int(rng.choice(used))
            if k < len(fields):
                fields[k] = " " * int(rng.integers(1, 3)) + fields[k] + " " * int(rng.integers(0, 3))   # a padded field
        line = glue.join(fields)
        if sep == ar.WHITESPACE and rng.random() < 0.2:
            line = "   " + line + " \t"
        out.append(line + ("\r\n" if rng.random() < 0.3 else "\n"))
        if rng.random() < 0.05:
            out.append(str(rng.choice(["", "   ", "\r"])) + "\n")          # a blank line
    data = "".join(out).encode()
    return data if final_newline else data.rstrip(b"\r\n")


def write_pipeline(fmt, directory, name=None):
    """the format's PDAL-style pipeline file in `directory`; returns its path"""
    sep = fmt["separator"]
    reader = {"type": "readers.text", "filename": fmt["filename"], "separator": sep, "skip": fmt["skip"], "header": sep.join(fmt["header"]),
              "usecols": sep.join(fmt["usecols"])}
    if fmt["na_values"] is not None:
        reader["na_values"] = fmt["na_values"]
    if fmt["converter"] is not None:
        new, a, op, b = fmt["converter"]
        reader["converters"] = {new: a + op + b}
    if fmt["dropcols"]:
        reader["dropcols"] = sep.join(fmt["dropcols"])
    stages = [reader]
    if fmt["reprojection"]:
        stages.append({"type": "filters.reprojection", "in_srs": fmt["reprojection"][0], "out_srs": fmt["reprojection"][1]})
    path = os.path.join(str(directory), (name or fmt["name"]) + ".json")
    with open(path, "w") as f:
        json.dump({"pipeline": stages}, f)
    return path


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def restated(fmt, data):
    return ar.read_table(data, fmt["separator"], fmt["skip"], fmt["header"], fmt["usecols"], fmt["na_values"])


def _pandas_table(pd, fmt, data):
    df = pd.read_csv(io.BytesIO(data), sep=fmt["separator"], header=fmt["skip"], names=fmt["header"], usecols=fmt["usecols"],
                     na_values=fmt["na_values"]).dropna()
    cols = [n for n in fmt["header"] if n in fmt["usecols"]]
    return df[cols].to_numpy(dtype=np.float64), cols


# ---- the restatement against pandas ----
@pytest.mark.parametrize("k", range(len(FORMATS)), ids=FORMAT_IDS)
def test_restatement_equals_pandas_on_the_eleven_formats(k):
    pd = pytest.importorskip("pandas")
    fmt = FORMATS[k]
    kept = 0
    for j, _ in enumerate(fmt["files"]):
        data = make_file(fmt, seed=100 * k + j, final_newline=(k + j) % 2 == 0)
        want, wcols = _pandas_table(pd, fmt, data)
        got, cols = restated(fmt, data)
        assert cols == wcols
        assert len(want) > 150
        assert same_bits(got, want), fmt["name"]
        kept += len(got)
    assert kept > 0


def test_generated_files_hold_what_they_claim():
    crlf = blank = short = padded = na = 0
    for k, fmt in enumerate(FORMATS):
        data = make_file(fmt, seed=k)
        crlf += data.count(b"\r\n")
        lines = ar.physical_lines(data)
        blank += sum(ar.is_blank(l, fmt["separator"]) for _, l in lines)
        body = [l for _, l in lines if not ar.is_blank(l, fmt["separator"])][fmt["skip"] + 1:]
        short += sum(len(ar.fields_of(l, fmt["separator"])) < len(fmt["header"]) for l in body)
        padded += sum(b" " in l for l in body) if fmt["separator"] != ar.WHITESPACE else 0
        na += sum(b"NaN" in l or (fmt["na_values"] or "\0").encode() in l for l in body)
        assert not make_file(fmt, seed=k, final_newline=False).endswith(b"\n")
    assert min(crlf, blank, short, padded, na) > 20


@pytest.mark.parametrize("sep", [",", "\t", ar.WHITESPACE], ids=["comma", "tab", "whitespace"])
def test_blank_lines_against_pandas(sep):
    pd = pytest.importorskip("pandas")
    glue = " " if sep == ar.WHITESPACE else sep
    names = ["a", "b", "c"]
    row = lambda *v: glue.join(str(x) for x in v)   # noqa: E731

    def both(data, skip=0):
        df = pd.read_csv(io.BytesIO(data), sep=sep, header=skip, names=names, usecols=names)
        full = df.to_numpy(dtype=np.float64)
        got, _ = ar.read_table(data, sep, skip, names, names)
        assert same_bits(got, df.dropna().to_numpy(dtype=np.float64)), data
        return full

    head = row("h1", "h2", "h3") + "\n"
    body = row(1, 2, 3) + "\n" + row(4, 5, 6) + "\n"
    # a spaces-only line is blank for every separator: it neither makes a row nor counts towards skip
    assert len(both((head + row(1, 2, 3) + "\n   \n" + row(4, 5, 6) + "\n").encode())) == 2
    assert len(both(("   \n" + head + "  \n" + head + body).encode(), skip=1)) == 2
    # a tabs-only line: blank for ',' and whitespace, a row of NaNs for the tab separator
    full = both((head + row(1, 2, 3) + "\n\t\t\n" + row(4, 5, 6) + "\n").encode())
    assert len(full) == (3 if sep == "\t" else 2)
    if sep == "\t":
        assert np.isnan(full[1]).all()
    if sep != ar.WHITESPACE:
        # separators only: a row of NaNs, and it counts towards skip
        full = both((head + row(1, 2, 3) + "\n" + sep + sep + "\n" + row(4, 5, 6) + "\n").encode())
        assert len(full) == 3 and np.isnan(full[1]).all()
        assert len(both((sep + sep + "\n" + head + body).encode(), skip=1)) == 2
        assert len(both((head + head + body).encode(), skip=1)) == 2


def test_header_equal_skip_loses_the_first_data_row():
    """the reference's quirk: `header=skip` with skip = 1 and ONE header line takes the first data row for the header"""
    got, _ = ar.read_table(b"x,y,z\n1,2,3\n4,5,6\n", ",", 1, ["x", "y", "z"], ["x", "y", "z"])
    assert got.tolist() == [[4.0, 5.0, 6.0]]
    pd = pytest.importorskip("pandas")
    df = pd.read_csv(io.BytesIO(b"x,y,z\n1,2,3\n4,5,6\n"), sep=",", header=1, names=["x", "y", "z"], usecols=["x", "y", "z"])
    assert df.to_numpy(dtype=float).tolist() == [[4.0, 5.0, 6.0]]


# ---- the grammar against float() ----
NUMBERS = ["0", "7", "-7", "+7", "12.5", "-12.5", "+.5", ".5", "-.25", "1.", "-1.", "-0", "-0.0", "+0", "0.000", "1e22", "1E-22", "1e23",
           "1e-23", "4.9e-324", "2.2250738585072014e-308", "1.7976931348623157e308", "1e400", "-1e400", "1e-400", "-1e-400", "1e+5",
           "1E5", "1.5e-3", "12345.678e2", "0.1", "0.3", "123456789012345", "1234567890123456", "12345678901234567",
           "1234567890123456789", "123456789012345678901234567890", "0.123456789012345", "0.1234567890123456", "0.12345678901234567",
           ".1234567890123456789", "0.123456789012345678901234567890", "9007199254740992", "9007199254740993", "9007199254740993e-5",
           "00000000000000000000001.5", "0.00000000000000000000000000015", "1e0000000000000000000001", "0e999999999", "123456.789012",
           "-75.123456", "8.98846567431158e307", "6.0221409e23", "1.0e-10", "5e-1"]
INFINITIES = ["inf", "-inf", "+inf", "Inf", "INF", "iNf", "infinity", "-Infinity", "+INFINITY", "InFiNiTy"]
BAD = ["1d5", "0x10", "1_000", "1.5e", "abc", '"1"', "1e+", "-", "+", ".", "e5", "1.2.3", "1 2", "--1", "+-1", "1e5.0", "infinit", "nane",
       "+nan", "1,5", "NAN"]


@pytest.mark.parametrize("text", NUMBERS + INFINITIES)
def test_numbers_have_the_bits_of_float(text):
    got = ar.value_of(text.encode())
    want = float(text)
    assert struct.pack("<d", got) == struct.pack("<d", want)
    assert ar.value_of(b" \t" + text.encode() + b"  ") == want


def test_special_values():
    assert ar.value_of(b"1e400") == math.inf and ar.value_of(b"-1e400") == -math.inf
    assert ar.value_of(b"1e-400") == 0.0 and math.copysign(1.0, ar.value_of(b"-1e-400")) == -1.0
    assert math.copysign(1.0, ar.value_of(b"-0")) == -1.0
    for digits in (15, 16, 17, 19, 30):
        m = ("1234567890" * 3)[:digits]
        for text in (m, "0." + m, m[:3] + "." + m[3:] + "e-7"):
            assert struct.pack("<d", ar.value_of(text.encode())) == struct.pack("<d", float(text))


@pytest.mark.parametrize("text", ar.DEFAULT_NA)
def test_every_default_na_string_is_nan(text):
    assert math.isnan(ar.value_of(text.encode()))
    pd = pytest.importorskip("pandas")
    df = pd.read_csv(io.BytesIO(b"1,2\n" + text.encode() + b",3\n"), sep=",", header=None, names=["a", "b"])
    assert math.isnan(df["a"].to_numpy(dtype=float)[1])


def test_na_values_are_compared_byte_for_byte():
    assert math.isnan(ar.value_of(b"*", ("*",))) and math.isnan(ar.value_of(b"-9999", ["-9999"]))
    assert ar.value_of(b"-9999.0", ["-9999"]) == -9999.0      # pandas' numeric comparison is NOT built
    with pytest.raises(ValueError):
        ar.value_of(b"*")


@pytest.mark.parametrize("text", BAD)
def test_anything_else_raises(text):
    with pytest.raises(ValueError):
        ar.value_of(text.encode())


def test_errors_name_the_first_line_and_the_column():
    data = b"h\nx,y\n1,2\n\n3,oops\n4,bad\n"
    with pytest.raises(ValueError, match=r"line 5: column 'b'"):
        ar.read_table(data, ",", 1, ["a", "b"], ["a", "b"])
    got, _ = ar.read_table(data, ",", 1, ["a", "b"], ["a"])     # junk in an unused field is accepted
    assert got.tolist() == [[1.0], [3.0], [4.0]]
    with pytest.raises(ValueError, match=r"line 2: 3 fields"):
        ar.read_table(b"h\n1,2,3\n", ",", 0, ["a", "b"], ["a"])
    got, _ = ar.read_table(b"h\n1\n2,3\n", ",", 0, ["a", "b"], ["a", "b"])     # a short line: NaN, dropped
    assert got.tolist() == [[2.0, 3.0]]


# ---- plumbing ----
@pytest.mark.parametrize("k", range(len(FORMATS)), ids=FORMAT_IDS)
def test_parse_pipeline_accepts_the_eleven_pipelines(k, tmp_path):
    from deepbedmap_amd import ascii_table as at

    fmt = FORMATS[k]
    reader, srs = at.parse_pipeline(write_pipeline(fmt, tmp_path))
    assert reader.separator == fmt["separator"] and reader.skip == fmt["skip"] and list(reader.names) == fmt["header"]
    assert list(reader.usecols) == fmt["usecols"] and reader.converter == fmt["converter"] and reader.dropcols == fmt["dropcols"]
    assert reader.na_values == ((fmt["na_values"],) if fmt["na_values"] else ()) and reader.filename == fmt["filename"]
    assert srs == fmt["reprojection"]
    plan = at.xyz_plan(reader)
    cols = at.table_columns(reader)
    assert cols == [n for n in fmt["header"] if n in fmt["usecols"]]
    if fmt["converter"]:   # Y, X, ELEVATION, BOTTOM -> x = X, y = Y, z = ELEVATION - BOTTOM
        assert plan == [(1, None, 0), (0, None, 0), (2, "-", 3)]
    else:
        assert [p[1] for p in plan] == [None] * 3 and [cols[p[0]] for p in plan] == sorted(cols)


def test_parse_pipeline_refuses_what_the_dialect_does_not_cover(tmp_path):
    from deepbedmap_amd import ascii_table as at

    dc8 = FORMATS[3]
    for k, expr in enumerate(["ELEVATION*BOTTOM", "ELEVATION-BOTTOM-SURFACE", "abs(BOTTOM)", "ELEVATION-1", "__import__('os')"]):
        bad = dict(dc8, converter=("Z", expr, "", ""))
        with pytest.raises(ValueError, match="converter"):
            at.parse_pipeline(write_pipeline(bad, tmp_path, "conv%d" % k))
    with pytest.raises(ValueError, match="three columns"):
        at.parse_pipeline(write_pipeline(dict(dc8, dropcols=("ELEVATION",)), tmp_path, "four"))
    with pytest.raises(ValueError, match="usecols"):
        at.parse_pipeline(write_pipeline(dict(dc8, usecols=["X", "Y", "ELEVATION", "DEPTH"]), tmp_path, "unknown"))
    with pytest.raises(ValueError, match="separator"):
        at.parse_pipeline(write_pipeline(dict(FORMATS[9], separator=";"), tmp_path, "semicolon"))
    with pytest.raises(ValueError, match="reprojected"):
        at.parse_pipeline(write_pipeline(dict(dc8, reprojection=("EPSG:4326", "EPSG:3413")), tmp_path, "north"))
    with pytest.raises(ValueError, match="skip"):
        at.parse_pipeline(write_pipeline(dict(dc8, skip=-1), tmp_path, "skip"))


def test_python_constants_equal_the_header():
    from deepbedmap_amd import ascii_table as at

    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    header = {k: int(v) for k, v in re.findall(r"\b(DBM_TEXT_[A-Z_]+)\s*=\s*(\d+)", text)}
    for name in ("TILE_BYTES", "THREADS", "SEP_WHITESPACE", "MAX_FIELDS", "MAX_NA", "MAX_NA_BYTES"):
        assert getattr(at, "TEXT_" + name) == header["DBM_TEXT_" + name], name
    assert at.TEXT_TILE_BYTES % (16 * at.TEXT_THREADS) == 0 and at.TEXT_TILE_BYTES // at.TEXT_THREADS == 64
    assert at.DEFAULT_NA == ar.DEFAULT_NA and at.WHITESPACE == ar.WHITESPACE


def test_new_symbols_are_bound_and_cite_the_reference():
    from deepbedmap_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    for name in ("dbm_text_count_lines", "dbm_text_parse", "dbm_text_columns"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        i = text.index("int " + name + "(")
        assert "data_prep.py:298-305" in text[max(0, i - 9000):i], name
    import deepbedmap_amd as dbm

    for name in ("ascii_to_xyz", "parse_pipeline", "read_text_table", "TextReader"):
        assert hasattr(dbm, name)
    src = open(os.path.join(ROOT, "deepbedmap_amd", "ascii_table.py")).read()
    assert re.search(r"^\s*(import|from)\s+pandas", src, re.M) is None     # the package imports no pandas


def test_no_gpu_means_dbm_error(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import deepbedmap_amd as dbm

    reader = dbm.TextReader(",", 0, ["a", "b"], ["a", "b"])
    with pytest.raises(dbm.DbmError):
        dbm.read_text_table(b"h\n1,2\n", reader)
    fmt = FORMATS[9]
    with open(os.path.join(str(tmp_path), fmt["files"][0]), "wb") as f:
        f.write(make_file(fmt, 1, lines=5))
    with pytest.raises(dbm.DbmError):
        dbm.ascii_to_xyz(write_pipeline(fmt, tmp_path))
    with pytest.raises(ValueError):   # (what the host can refuse it refuses before it needs a GPU)
        dbm.read_text_table(b"1;2\n", dbm.TextReader(";", 0, ["a", "b"], ["a"]))
