"""CPU-side checks of the drop-in boundary: libdbm.so loads, exports every symbol include/dbm.h declares, and
the product path fails loudly (no CPU fallback) when no MI355X is visible."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from deepbedmap_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dbm_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound(built):
    import ctypes

    lib = ctypes.CDLL(built.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 35
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/dbm.h but not exported by libdbm.so"
    bound = set(built.SIGNATURES) | {"dbm_last_error"}
    assert set(syms) == bound, set(syms) ^ bound


def test_flag_values_of_the_header_and_the_bindings_agree(built):
    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"\b(DBM_[A-Z0-9_]+)\s*=\s*(\d+)", text)}
    for name in ("DEVICE_PTRS", "KEEP_GRAPH", "BN_TRAIN", "BF16", "ONE_GEN_FORWARD"):
        assert flags["DBM_" + name] == getattr(built, name), name
    used = [flags["DBM_" + n] for n in ("DEVICE_PTRS", "KEEP_GRAPH", "BN_TRAIN", "BF16", "ONE_GEN_FORWARD")]
    assert len(set(used)) == len(used) and all(v & (v - 1) == 0 for v in used)  # distinct single bits


def test_every_entry_point_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    for name in ("dbm_gen_create", "dbm_disc_create", "dbm_gen_forward", "dbm_disc_forward", "dbm_generator_loss",
                 "dbm_discriminator_loss", "dbm_adam_setup", "dbm_adam_update", "dbm_discriminator_step",
                 "dbm_generator_step", "dbm_model_cleargrads", "dbm_model_count_params"):
        i = text.index(name + "(")
        assert re.search(r"(srgan_train|deepbedmap)\.py:\d+", text[max(0, i - 1800):i]), name


def test_no_gpu_means_loud_failure(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import deepbedmap_amd as dbm

    with pytest.raises(dbm.DbmError, match="no HIP device|no CPU fallback|dbm_init"):
        dbm.Context(0)
    with pytest.raises(dbm.DbmError):
        dbm.GeneratorModel()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "deepbedmap_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_product_library_has_no_work_skipping_switches(built):
    """switches that skip work (results then wrong) must not ship.  They are compiled only with -DDBM_MEASURE
    into libdbm_measure.so (tools/build_measure.sh); the product library does not even contain their names, the package loads another
    library only when DBM_LIB points at a libdbm_measure.so, and bench.py refuses to run with DBM_LIB or one of the switches set."""
    from deepbedmap_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"DBM_ABL_SKIP", b"DBM_NO_WGRAD", b"DBM_TFB_ABL", b"DBM_CL16_ABL", b"DBM_ABL_NOPACK", b"ABL_SKIP", b"NO_WGRAD", b"TFB_ABL",
                 b"CL16_ABL", b"ABL_NOPACK"):
        assert name not in blob, name
    # switched-off variants that lost their A/B in round 3 are gone as well
    for name in (b"DBM_TWIN_EARLY", b"DBM_ITER_TAIL", b"DBM_PF_PRIORITY", b"DBM_CL16_SMALL", b"DBM_IGEMM_LDS"):
        assert name not in blob, name
    import bench

    assert set(("DBM_ABL_SKIP", "DBM_NO_WGRAD", "DBM_TFB_ABL", "DBM_CL16_ABL", "DBM_ABL_NOPACK", "DBM_LIB")) <= set(bench.WORK_SKIPPING_ENV)
    assert _lib.library_path({}) == _lib.LIB_PATH
    with pytest.raises(_lib.DbmError, match="libdbm_measure.so"):
        _lib.library_path({"DBM_LIB": "/tmp/some_other_library.so"})
    with pytest.raises(_lib.DbmError, match="libdbm_measure.so"):
        _lib.library_path({"DBM_LIB": _lib.LIB_PATH})   # (not even the product library under that switch)


def test_environment_switches_of_the_product_library_are_few_and_exercised(built):
    """VERDICT round 5 #8a (knob sprawl: 64 getenv("DBM_*") in libdbm.so).  The tuning switches (launch-size rules, kernel-form
    overrides: DBM_IGEMM_*, DBM_WGRAD_*, ...) are gone: their defaults are constants of the sources.  What the PRODUCT library still
    reads -- every DBM_* name in its strings that is not an API flag of include/dbm.h -- must stay at or below 23 names, and every one of them must
    be set by a parity test under tests/ (a code path the test suite runs) -- not merely mentioned by a tool."""
    blob = open(built.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"DBM_[A-Z0-9_]+", blob))
    header = open(os.path.join(ROOT, "include", "dbm.h")).read()
    api_names = set(re.findall(r"\b(DBM_[A-Z0-9_]+)\b", header)) | {"DBM_MAX_TAPS", "DBM_HIP", "DBM_CHECK"}
    knobs = sorted(names - api_names)
    assert len(knobs) <= 23, knobs
    tests_src = "".join(open(os.path.join(ROOT, "tests", f)).read() for f in os.listdir(os.path.join(ROOT, "tests")) if f.endswith(".py"))
    this = open(__file__).read()
    tests_src = tests_src.replace(this, "")
    unexercised = [k for k in knobs if not re.search(r'"%s"|\b%s="' % (k, k), tests_src)]   # {"NAME": "v"} or NAME="v" (os.environ.update)
    assert not unexercised, f"switches read by libdbm.so that no test sets: {unexercised}"
    # ... and the tuning names are really gone from the product library
    for name in (b"DBM_IGEMM_", b"DBM_WGRAD_", b"DBM_CL16_SLOTS", b"DBM_TRUNK_SPLIT", b"DBM_ITER_AUX", b"DBM_DBWD_ORDER"):
        assert name not in blob, name
    # ... and so are the product schedules that lost their A/Bs (profiles/r5/ab_twin.txt, ab_conv_tile_classes_late.txt,
    # profiles/r6/ab_defer_eval.txt)
    for name in (b"DBM_ITER_DEFER_EVAL", b"DBM_ITER_EARLY_TWIN", b"DBM_CONV_TILE_9"):
        assert name not in blob, name


def test_sources_have_no_tuning_switch_layer():
    """The tuning layer (DBM_TUNE_GETENV: getenv in libdbm_measure.so, a null pointer in libdbm.so) is gone: every launch rule the
    product runs is what the sources say."""
    csrc = os.path.join(ROOT, "deepbedmap_amd", "csrc")
    offenders = [f for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f)) and "DBM_TUNE_GETENV" in open(os.path.join(csrc, f)).read()]
    assert not offenders, offenders
