"""No GPU: the stream entries of the C ABI as the header declares them, what they answer without a device, and the Python front's
two switches (api.use_torch_stream / api.use_own_stream).  The ordering itself is tests/test_gpu_streams.py's."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "lcg_hip.h")
CTYPE = {"int": C.c_int, "void *": C.c_void_p, "void": None}


def _prototype(name):
    """(return type, [argument types]) of `name` as the header spells them, comments removed."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*([a-z_ ]+?\*?)\s*" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, name
    ret = m.group(1).strip()
    ret = "void *" if ret.replace(" ", "") == "void*" else ret
    args = [a.strip() for a in m.group(2).split(",")]
    args = [] if args == ["void"] else ["void *" if "*" in a else a.split()[0] for a in args]
    return ret, args


def test_prototypes_match_the_header():
    from liblcg_amd import _lib
    assert _prototype("lcg_hip_set_stream") == ("int", ["void *"])
    assert _prototype("lcg_hip_get_stream") == ("void *", [])
    for name in ("lcg_hip_set_stream", "lcg_hip_get_stream"):
        ret, args = _prototype(name)
        assert _lib.SIGNATURES[name] == (CTYPE[ret], [CTYPE[a] for a in args]), (name, _lib.SIGNATURES[name])


def _exported():
    """Every function the header declares, in its order (the callback TYPES are typedefs: `(*name)(`, never `name(`)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+[ \*]+(c?lcg_hip_[a-z0-9_]+)\s*\(", src, flags=re.M)
    assert len(names) == len(set(names)) and len(names) > 150, len(names)
    for name in ("lcg_hip_set_stream", "lcg_hip_get_stream", "lcg_hip_init", "clcg_hip_lpcg_multi_c64"):
        assert name in names and _prototype(name), name         # (the spelling _prototype reads is found here too)
    return names


def _mentions(text, what):
    """`what` in text, not as a part of a longer identifier (lcg_hip_spmv is not named by lcg_hip_spmv_op)."""
    pat = r"(?<![A-Za-z0-9_])" + re.escape(what) + (r"(?![A-Za-z0-9_])" if re.match(r"[A-Za-z0-9_]", what[-1]) else "")
    return re.search(pat, text) is not None


def _api_body(method):
    """The text of liblcg_amd.api's function or method `method`."""
    src = open(os.path.join(ROOT, "liblcg_amd", "api.py")).read()
    m = re.search(r"^( *)def " + re.escape(method) + r"\(.*?(?=^\1(?:def |class |@)|^(?:def |class |@)|\Z)", src, flags=re.M | re.S)
    assert m, method
    return m.group(0)


def stream_coverage_gaps(table, exported):
    """What is wrong with a coverage table (tests/stream_cases.py: STREAM_COVERAGE) -- a list of plain sentences, empty when the
    table is complete and every covered entry is found where the table says."""
    gaps = [f"{n}: exported by include/lcg_hip.h, missing from the table" for n in exported if n not in table]
    gaps += [f"{n}: in the table, not exported by include/lcg_hip.h" for n in table if n not in exported]
    files = {}

    def text_of(name):
        if name not in files:
            path = os.path.join(ROOT, "tests", name)
            files[name] = open(path).read() if os.path.exists(path) else None
        return files[name]
    for entry, where in table.items():
        if isinstance(where, tuple) and where[0] == "exempt":
            if len(where) != 2 or len(where[1].split()) < 2:
                gaps.append(f"{entry}: exempt without a reason")
            continue
        test_id, text, helper = (where, entry, None) if isinstance(where, str) else (tuple(where) + (None,))[:3]
        fname, _, func = test_id.partition("::")
        src = text_of(fname)
        if src is None or not re.search(r"^def " + re.escape(func) + r"\(", src, flags=re.M):
            gaps.append(f"{entry}: no test {func} in tests/{fname}")
            continue
        if "pytest.mark.gpu" not in src or "stream_cases" not in src:
            gaps.append(f"{entry}: tests/{fname} is no GPU test of the late-input pattern")
        spelled = src
        if helper is not None:
            spelled = text_of(helper)
            if spelled is None or not _mentions(src, helper[:-3]):
                gaps.append(f"{entry}: tests/{fname} does not use tests/{helper}")
                continue
        if not _mentions(spelled, text):
            gaps.append(f"{entry}: tests/{helper or fname} does not mention {text}")
        elif not _mentions(text, entry):      # a call of the Python front: that method must be the one that calls the entry
            method = re.search(r"([A-Za-z_0-9]+)\(?$", text).group(1)
            if not _mentions(_api_body(method), entry):
                gaps.append(f"{entry}: liblcg_amd.api.{method} does not call it")
    return gaps


def test_every_exported_entry_has_a_stream_test_or_a_reason():
    """tests/stream_cases.py: STREAM_COVERAGE names, for every entry the header exports, the test that runs it on a caller's stream
    under the late-input pattern, or the reason why none does.  An entry added to the header without a line there fails here, on a
    machine without a GPU; so does a line whose test is gone or no longer mentions the entry."""
    import stream_cases as st
    from liblcg_amd import _lib
    exported = _exported()
    assert set(exported) == set(_lib.SIGNATURES), set(exported) ^ set(_lib.SIGNATURES)
    gaps = stream_coverage_gaps(st.STREAM_COVERAGE, exported)
    assert not gaps, "\n".join(gaps)


@pytest.mark.parametrize("gone", ["lcg_hip_dense_ata_multi", "clcg_hip_spmm_c64", "clcg_hip_dense_lpcg_multi"])
def test_the_table_check_sees_a_missing_or_misplaced_entry(gone):
    """The check itself: a k-wide entry taken out of the table, pointed at a test that does not exist, or at one that does not
    mention it, is reported."""
    import stream_cases as st
    exported = _exported()
    table = dict(st.STREAM_COVERAGE)
    del table[gone]
    assert stream_coverage_gaps(table, exported) == [f"{gone}: exported by include/lcg_hip.h, missing from the table"]
    table[gone] = st.NEW + "::test_that_was_never_written"
    assert stream_coverage_gaps(table, exported) == [f"{gone}: no test test_that_was_never_written in tests/{st.NEW}"]
    table[gone] = st.OLD + "::test_level_one"
    assert stream_coverage_gaps(table, exported) == [f"{gone}: tests/{st.OLD} does not mention {gone}"]
    table[gone] = ("exempt", "")
    assert stream_coverage_gaps(table, exported) == [f"{gone}: exempt without a reason"]


def test_the_header_and_the_guide_state_both_rules():
    """The contract next to the prototype and in INTEGRATION.md: the new stream waits for the previous one; the previous one must
    still exist."""
    src = open(HEADER).read()
    at = src.index("int  lcg_hip_set_stream(")
    note = " ".join(src[max(0, at - 1200):at].split())
    assert "waits" in note and "previous stream" in note and "must still exist" in note and "does nothing" in note, note
    guide = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert "lcg_hip_set_stream" in guide and "must still exist" in guide and "waits" in guide


def test_without_a_device_the_entries_say_so():
    import torch
    from liblcg_amd import _lib
    lib = _lib.load()
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    assert lib.lcg_hip_set_stream(None) == -2001                # LCG_HIP_E_NO_DEVICE
    assert lib.lcg_hip_set_stream(C.c_void_p(1)) == -2001
    assert b"no" in lib.lcg_hip_last_error().lower()
    assert lib.lcg_hip_get_stream() is None                     # NULL
    assert lib.lcg_hip_synchronize() == -2001


def test_the_python_front_has_both_switches():
    import torch
    from liblcg_amd import api
    assert callable(api.use_own_stream) and callable(api.use_torch_stream)
    if not torch.cuda.is_available():
        with pytest.raises(api.LcgHipError):                    # a missing device is an error, not a silent no-op
            api.use_own_stream()
