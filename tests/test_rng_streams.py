"""The Philox stream ids are stated once, in ofighters_amd/csrc/ofx_rng.h: pairwise distinct, exactly 0 .. 11, defined
nowhere else in the library, and equal to what the independent restatements (the Python oracles of tests/ and
oracle/ofx_oracle.c) key their draws on.  Two streams with one id would give correlated draws that no parity test
notices, since both sides would agree.  CPU only: the files are read as text."""
import glob
import os
import re

from tests import augment_oracle, boltzmann_oracle, evolution_oracle, global_sample_oracle, per_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofighters_amd", "csrc")
NAMES = ("BOT", "RESET", "EXPLORE", "REPLAY", "PER", "GLOBAL", "BOLTZMANN_PTR", "BOLTZMANN_ACT", "AUGMENT", "EVOLVE",
         "MUTATE", "FRESH")


def _header_ids():
    text = open(os.path.join(CSRC, "ofx_rng.h")).read()
    found = re.findall(r"^\s*OFX_STREAM_(\w+)\s*=\s*(\d+)\s*,", text, re.M)
    ids = {name: int(value) for name, value in found}
    assert len(ids) == len(found), "a stream name is defined twice"
    return ids


def test_ids_are_distinct_and_exactly_0_to_11():
    ids = _header_ids()
    assert set(ids) == set(NAMES)
    assert sorted(ids.values()) == list(range(12))


def test_no_other_file_defines_a_stream():
    """A definition is `#define OFX_STREAM_X` or an enumerator `OFX_STREAM_X = n`; uses (arguments, comments) are not."""
    define = re.compile(r"#\s*define\s+OFX_STREAM_\w+|\bOFX_STREAM_\w+\s*=[^=]")
    files = [f for f in glob.glob(os.path.join(CSRC, "*")) if f.endswith((".h", ".hip", ".cpp", ".c", ".hpp"))]
    assert os.path.join(CSRC, "ofx_rng.h") in files and len(files) > 10
    for f in files:
        if os.path.basename(f) != "ofx_rng.h":
            assert not define.search(open(f).read()), os.path.basename(f)
    public = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert not define.search(public)


def test_ids_equal_the_python_oracles():
    ids = _header_ids()
    assert ids["PER"] == per_oracle.STREAM_PER
    assert ids["GLOBAL"] == global_sample_oracle.STREAM_GLOBAL
    assert ids["AUGMENT"] == augment_oracle.STREAM_AUGMENT
    assert (ids["BOLTZMANN_PTR"], ids["BOLTZMANN_ACT"]) == (boltzmann_oracle.STREAM_PTR, boltzmann_oracle.STREAM_ACT)
    assert (ids["EVOLVE"], ids["MUTATE"], ids["FRESH"]) == (evolution_oracle.STREAM_EVOLVE, evolution_oracle.STREAM_MUTATE,
                                                           evolution_oracle.STREAM_FRESH)


def test_ids_equal_the_c_oracle():
    text = open(os.path.join(ROOT, "oracle", "ofx_oracle.c")).read()
    orc = {name: int(value) for name, value in re.findall(r"^#define ORC_STREAM_(\w+)\s+(\d+)u?\s*$", text, re.M)}
    ids = _header_ids()
    assert set(orc) == {"BOT", "RESET", "EXPLORE"}
    for name, value in orc.items():
        assert ids[name] == value, name
