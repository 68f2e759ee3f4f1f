"""`geotiff.inflate` -- the device inflate decoder's loop run with one lane on the host (dbm_inflate; tiff_inflate.hip) --
against `zlib.decompress` and the plain restatement in tests/inflate_restatement.py.  Every comparison is on bytes.  What each input
exercises is asserted through the restatement's statistics, so a zlib that compresses differently shows up as a failed assertion
about the input, not as a silent loss of coverage."""
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inflate_restatement as rs  # noqa: E402

import deepbedmap_amd as dbm  # noqa: E402
from deepbedmap_amd import geotiff  # noqa: E402


def twin(stream, nbytes):
    return geotiff.inflate(stream, nbytes).tobytes()


@pytest.fixture(scope="module")
def decoded():
    """name -> (bytes, statistics) of the restatement, once."""
    return {name: rs.inflate(stream) for name, (stream, _) in rs.zlib_streams().items()}


@pytest.mark.parametrize("name", ["a_level0", "a_level6", "a_fixed", "b_zeros", "c_huffman_only", "d_full_flush", "e_wbits9", "f_one_byte"])
def test_streams_of_zlib(decoded, name):
    stream, raw = rs.zlib_streams()[name]
    back, st = decoded[name]
    assert back == raw and zlib.decompress(stream) == raw
    if name == "a_level0":
        assert len(raw) == 131072 and st["types"] == [0, 0, 0]
    elif name == "a_level6":
        assert st["types"] == [2] * 7 and st["largest_distance"] > 32000
    elif name == "a_fixed":
        assert set(st["types"]) == {1}
    elif name == "b_zeros":
        assert len(st["types"]) == 1 and st["largest_distance"] == 1 and st["matches_258"] > 500
    elif name == "c_huffman_only":
        assert len(raw) == 60000 and st["matches"] == 0 and st["longest_lit"] >= 13 and st["longest_lit_used"] >= 13
    elif name == "d_full_flush":
        assert 0 in st["stored_lengths"] and 0 in st["types"] and 2 in st["types"]   # the empty stored block, then realignment
    elif name == "e_wbits9":
        assert stream[0] >> 4 == 1 and 0 < st["largest_distance"] <= 512
    else:
        assert len(raw) == 1
    assert twin(stream, len(raw)) == raw


@pytest.mark.parametrize("name", ["distance_32768_at_32768", "distance_3_length_258", "distance_1_length_3_at_1", "match_258_across_64",
                                  "one_distance_code", "no_distance_code", "literal_code_of_15_bits"])
def test_streams_zlib_never_emits(name):
    stream, raw = rs.token_streams()[name]
    back, st = rs.inflate(stream)
    assert back == raw == zlib.decompress(stream)
    if name == "distance_32768_at_32768":
        assert st["largest_distance"] == 32768 and len(raw) == 32768 + 3 and raw[-3:] == raw[:3]
    elif name == "distance_3_length_258":
        assert raw == b"abc" * 87 and st["matches_258"] == 1
    elif name == "distance_1_length_3_at_1":
        assert raw == bytes([5]) * 4
    elif name == "match_258_across_64":
        assert len(raw) == 54 + 258 + 3 and st["matches_258"] == 1
    elif name == "one_distance_code":
        assert st["types"] == [2] and st["dist_codes"] == [1] and st["longest_dist"] == 1 and st["matches"] == 3
    elif name == "no_distance_code":
        assert st["types"] == [2] and st["dist_codes"] == [0] and st["matches"] == 0
    else:
        assert st["types"] == [2] and st["longest_lit_used"] == 15
    assert twin(stream, len(raw)) == raw


def test_refusals_are_zlibs():
    good, raw = rs.zlib_streams()["a_level6"]
    cases = dict(rs.refusals())
    cases["distance_32768_at_32767"] = rs.token_streams()["distance_32768_at_32767"][0]
    assert set(cases) == {"cut_in_half", "trailer_flipped", "btype_3", "nlen", "fdict", "cm_7", "junk_behind", "distance_32768_at_32767"}
    for name, stream in cases.items():
        if name == "junk_behind":
            assert zlib.decompress(stream) == raw and rs.inflate(stream)[0] == raw and twin(stream, len(raw)) == raw
            continue
        with pytest.raises(zlib.error):
            zlib.decompress(stream)
        with pytest.raises(rs.Malformed):
            rs.inflate(stream)
        with pytest.raises(dbm.DbmError):
            twin(stream, 1000 if name == "nlen" else 32770 if name.startswith("distance") else len(raw))


def test_sizes_other_than_the_blocks():
    """More output than asked for is malformed, as in the LZW stage; less is reported as a size that does not match."""
    stream, raw = rs.zlib_streams()["a_level6"]
    for nbytes in (len(raw) - 1, len(raw) // 2, 0, len(raw) + 1):
        with pytest.raises(dbm.DbmError):
            twin(stream, nbytes)
    assert twin(zlib.compress(b""), 0) == b""
    for junk in (b"", b"\x78", b"\x78\x9c", bytes(64), b"\xff" * 64):
        with pytest.raises(dbm.DbmError):
            twin(junk, 16)


def test_the_writers_keep_refusing_deflate(tmp_path):
    a = np.zeros((1, 8, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="unsupported compression"):
        dbm.save_array_to_grid(str(tmp_path / "x"), (0.0, 0.0, 8.0, 8.0), a, compression="deflate")
