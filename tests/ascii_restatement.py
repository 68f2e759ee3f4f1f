"""Pure-Python restatement of the text dialect (DESIGN.md "Reading text tables"; dbm_text_count_lines, dbm_text_parse, dbm_text_columns
in include/dbm.h): split the lines, split the fields, then `float()`.  Not collected by pytest: tests/test_ascii_host.py pins it bit for
bit to `pandas.read_csv(...).dropna()` and to `float()`, tests/test_gpu_ascii.py compares the kernels with it.  No pandas here."""
import re

import numpy as np

WHITESPACE = "\\s+"
DEFAULT_NA = ("", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA", "NULL",
              "NaN", "None", "n/a", "nan", "null")
NUMBER = re.compile(rb"[+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?")
INFINITY = re.compile(rb"[+-]?(inf|infinity)", re.IGNORECASE)


def physical_lines(data):
    """[(1-based line number, content)]: lines end at '\\n', one '\\r' before it is dropped, a last line without '\\n' counts"""
    pieces = bytes(data).split(b"\n")
    last = pieces.pop()
    lines = [p[:-1] if p.endswith(b"\r") else p for p in pieces]
    if last:
        lines.append(last)   # (no '\n' behind it: a '\r' at its end stays)
    return list(enumerate(lines, start=1))


def is_blank(line, separator):
    """nothing but spaces and tabs -- a tab is not blank space when it is the separator"""
    return line.strip(b" " if separator == "\t" else b" \t") == b""


def fields_of(line, separator):
    if separator == WHITESPACE:
        return [f for f in re.split(rb"[ \t]+", line) if f]
    return line.split(separator.encode())


def value_of(field, na_values=()):
    """a trimmed field -> float (NaN for an NA string); ValueError for anything outside the grammar"""
    f = field.strip(b" \t")
    if f in set(s.encode() for s in DEFAULT_NA + tuple(na_values)):
        return float("nan")
    if INFINITY.fullmatch(f) or NUMBER.fullmatch(f):
        return float(f.decode("ascii"))
    raise ValueError(f"{f!r} is neither a number nor an NA string")


def count_lines(data, separator):
    lines = physical_lines(data)
    return len(lines), sum(not is_blank(l, separator) for _, l in lines)


def read_table(data, separator, skip, names, usecols, na_values=()):
    """(table (n, nuse) float64, the used names in file order) as read_csv(sep, header=skip, names, usecols, na_values).dropna() gives
    them; ValueError("line N: ...") for the first line, in file order, with a bad used field or more fields than names"""
    na_values = (na_values,) if isinstance(na_values, str) else tuple(na_values or ())
    cols = [n for n in names if n in usecols]
    rows = []
    inked = [(n, l) for n, l in physical_lines(data) if not is_blank(l, separator)]
    for number, line in inked[skip + 1:]:
        fields = fields_of(line, separator)
        if len(fields) > len(names):
            raise ValueError(f"line {number}: {len(fields)} fields, the header names {len(names)}")
        row = []
        for k, name in enumerate(names):
            if name in usecols:
                try:
                    row.append(value_of(fields[k] if k < len(fields) else b"", na_values))
                except ValueError as e:
                    raise ValueError(f"line {number}: column {name!r}: {e}") from None
        if not any(v != v for v in row):
            rows.append(row)
    return np.array(rows, dtype=np.float64).reshape(len(rows), len(cols)), cols


def to_xyz(table, cols, converter=None, dropcols=()):
    """the steps behind the read: NEW = A op B, dropcols removed, the three remaining columns sorted by name -> (n, 3) x, y, z"""
    data = {c: table[:, k] for k, c in enumerate(cols)}
    if converter is not None:
        new, a, op, b = converter
        data[new] = data[a] + data[b] if op == "+" else data[a] - data[b]
    for c in dropcols:
        del data[c]
    assert len(data) == 3, sorted(data)
    return np.stack([data[c] for c in sorted(data)], axis=1) if len(table) else np.empty((0, 3))
